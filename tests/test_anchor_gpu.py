"""Anchored alignment on the device (csrc/anchor.hip behind mp_anchor_set / mp_anchor_align) against the yardstick of
tests/anchor_ref.py on the cases of tests/anchor_cases.py: every query's row bytes, score, d0, counts, first / last column, status and
ops must be equal.  Then the batching, and the drop-in end to end: a seeded synthetic alignment is split into a 16-row seed and
unaligned queries, put together again and handed to the core step."""
import os
import subprocess
import sys

import numpy as np
import pytest

import anchor_cases as cases
from conftest import REPO
from multiprime_amd._abi import ANCHOR_MAX_LEN, MprimeError
from multiprime_amd.anchor import AnchoredAlignment
from multiprime_amd.synth import synth_block, to_fasta

FIELDS = ("score", "d0", "n_match", "n_ins", "n_del", "first_col", "last_col", "status")


@pytest.fixture(scope="module")
def truth():
    """The yardstick's results of every group, computed once."""
    groups = cases.all_groups()
    return groups, [cases.yardstick(g) for g in groups]


def pack(queries):
    raw = [q.encode() for q in queries]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw), np.uint8), off


def device(ctx, g, queries=None):
    ctx.anchor_set(g["anchor"].encode(), g["col"], g["width"], **g["params"])
    rows, meta, ops = ctx.anchor_align(*pack(g["queries"] if queries is None else queries), want_ops=True)
    return [dict(zip(FIELDS, mt[:8]), row=row.tobytes().decode(), ops=op.decode()) for row, mt, op in zip(rows, meta.tolist(), ops)]


def same(got, want, what):
    assert len(got) == len(want), what
    for q, (a, b) in enumerate(zip(got, want)):
        for key in FIELDS + ("ops", "row"):
            assert a[key] == b[key], (what, q, key, a[key], b[key])


@pytest.mark.gpu
def test_every_group_equals_the_yardstick(hip_lib, truth):
    assert hip_lib.backend == "hip" and hip_lib.anchor
    ctx = hip_lib.context(0)
    try:
        for g, want in zip(*truth):
            same(device(ctx, g), want, g["name"])
        batches = ctx.anchor_stats()[1]["batches"]
        assert batches == 1
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_queries", (1, 63, 64, 65, 200))
def test_results_do_not_depend_on_the_batch(n_queries, hip_lib, truth, monkeypatch):
    g, want = next((g, w) for g, w in zip(*truth) if g["name"] == "random200")
    monkeypatch.setenv("MP_ANCHOR_BATCH", "64")
    ctx = hip_lib.context(0)
    try:
        same(device(ctx, g, g["queries"][:n_queries]), want[:n_queries], f"batch 64, {n_queries} queries")
        assert ctx.anchor_stats()[1]["batches"] == (n_queries + 63) // 64
        # without ops: the same rows and records
        rows, meta, ops = ctx.anchor_align(*pack(g["queries"][:n_queries]))
        assert ops is None and [r.tobytes().decode() for r in rows] == [w["row"] for w in want[:n_queries]]
        assert meta[:, :8].tolist() == [[w[k] for k in FIELDS] for w in want[:n_queries]]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_two_queries_at_the_length_limit(hip_lib, monkeypatch):
    """An anchor of ANCHOR_MAX_LEN bases on identity columns, a copy with substitutions and a fragment with three inserted bases: one wave
    per workgroup in the sweep and a vote histogram beyond 64 KiB.  The expectation comes from the planted homology
    (star_edge_cases.limit_case; tests/test_star.py holds the yardstick to it at 3000 bases)."""
    from star_edge_cases import limit_case
    monkeypatch.delenv("MP_ANCHOR_BATCH", raising=False)
    case = limit_case(ANCHOR_MAX_LEN)
    g = dict(anchor=case["anchor"], col=list(range(ANCHOR_MAX_LEN)), width=ANCHOR_MAX_LEN, params={}, queries=case["records"][1:])
    ctx = hip_lib.context(0)
    try:
        same(device(ctx, g), case["anchored"], "length limit")
        assert ctx.anchor_stats()[1]["batches"] == 1
    finally:
        ctx.close()


@pytest.mark.gpu
def test_refusals(hip_lib):
    ctx = hip_lib.context(0)
    try:
        with pytest.raises(MprimeError, match="no anchor"):
            ctx.anchor_width = 8
            ctx.anchor_align(*pack(["ACGT"]))
        ctx.anchor_set(b"ACGTACGT", list(range(8)), 8)
        data, off = pack(["ACGT", "AC"])
        off[2] = off[1]                                             # an empty query: named, nothing launched
        with pytest.raises(MprimeError, match="query 1"):
            ctx.anchor_align(data, off)
        with pytest.raises(MprimeError, match="band"):
            ctx.anchor_set(b"ACGT", [0, 1, 2, 3], 4, band=256)
        with pytest.raises(MprimeError, match="ascending"):
            ctx.anchor_set(b"ACGT", [0, 2, 1, 3], 4)
    finally:
        ctx.close()


def _split(tmp_path, rows, n_seed=16, mutate=None):
    seed, queries, original = tmp_path / "seed.tmsa", tmp_path / "queries.fa", tmp_path / "original.tmsa"
    original.write_bytes(to_fasta(rows))
    seed.write_bytes(to_fasta(rows[:n_seed]))
    with open(queries, "wb") as f:
        for i in range(n_seed, rows.shape[0]):
            q = rows[i][rows[i] != ord("-")].tobytes()
            f.write(b">s%07d\n" % i + (mutate(i, q) if mutate else q) + b"\n")
    return str(seed), str(queries), str(original)


def _quiet_ends(rows, n_seed):
    """The condition under which a substitution-only row is its own best alignment: at most one base differing from the anchor among its
    first and among its last eight.  (Two differing bases at the very end are the exception the rule makes: dropping the second-last
    base, 12, can let the last one match one column earlier, +5 for -4, and saves the other mismatch: +1.  Inside a row, or with one
    substitution, moving anything costs a gap and turns matches into chance.)  Checked on the input alone."""
    from multiprime_amd.anchor import anchor_of
    anchor = np.frombuffer(anchor_of(rows[:n_seed])[0], np.uint8)
    assert len(anchor) == rows.shape[1]
    differs = rows != anchor[None, :]
    return bool((differs[:, :8].sum(axis=1) <= 1).all() and (differs[:, -8:].sum(axis=1) <= 1).all())


def _core(hip_lib, inp, out):
    from multiprime_amd.core import NN_degenerate
    NN_degenerate(seq_file=inp, primer_length=18, coverage=0.8, number_of_dege_bases=4, score_of_dege_bases=10, raw_entropy_threshold=3.6,
                  product_len=100, position="1,2,-1", variation=1, distance=4, GC="0.2,0.7", nproc=1, outfile=out, library=hip_lib).run()
    return open(out, "rb").read()


@pytest.mark.gpu
def test_end_to_end_without_indels(hip_lib, tmp_path):
    rows = synth_block(0, 256, 400, 20, p_gap=0.0, edge_frac=0.0, p_iupac=0.0, block_rows=256)
    assert not (rows == ord("-")).any() and _quiet_ends(rows, 16) and (rows != rows[0]).sum() > 2000
    seed, queries, original = _split(tmp_path, rows)
    out = str(tmp_path / "out.tmsa")
    app = AnchoredAlignment(seed, queries, out, library=hip_lib).run()
    assert open(out, "rb").read() == open(original, "rb").read()
    assert all(m["status"] == 0 and m["n_ins"] == 0 and m["n_del"] == 0 for m in app.meta()) and len(app.ids()) == 240
    assert app.rows().shape == (240, 400) and open(out + ".unaligned.fa", "rb").read() == b""
    tsv = _core(hip_lib, out, str(tmp_path / "out.tsv"))
    assert tsv == _core(hip_lib, original, str(tmp_path / "original.tsv")) and tsv.count(b"\n") > 1


@pytest.mark.gpu
def test_end_to_end_with_indels(hip_lib, tmp_path):
    rows = synth_block(0, 256, 400, 22, p_gap=0.0, edge_frac=0.0, p_iupac=0.0, block_rows=256)
    rng = np.random.default_rng(5)

    def mutate(i, q):
        p, g = int(rng.integers(30, 360)), int(rng.integers(1, 6))
        return q[:p] + q[p + g:] if i % 2 else q[:p] + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), g)) + q[p:]

    seed, queries, _ = _split(tmp_path, rows, mutate=mutate)
    out = str(tmp_path / "out.tmsa")
    app = AnchoredAlignment(seed, queries, out, library=hip_lib).run()
    meta = app.meta()
    assert all(m["status"] == 0 for m in meta) and sum(m["n_del"] > 0 for m in meta) > 60 and sum(m["n_ins"] > 0 for m in meta) > 60
    lines = open(out, "rb").read().split(b"\n")
    assert len(lines) == 2 * 256 + 1 and all(len(x) == 400 for x in lines[1::2])
    assert _core(hip_lib, out, str(tmp_path / "out.tsv")).count(b"\n") > 1


@pytest.mark.gpu
def test_the_script(tmp_path):
    rows = synth_block(0, 40, 200, 23, p_gap=0.0, edge_frac=0.0, p_iupac=0.0, block_rows=64)
    rows[:, :] = np.where(np.isin(rows, (ord("A"), ord("G"))), ord("C"), rows)      # a C / T alignment: a query of A and G is rejected
    assert _quiet_ends(rows, 8)
    seed, _, original = _split(tmp_path, rows, n_seed=8)
    queries2 = tmp_path / "q2.fa"
    with open(queries2, "wb") as f:
        for i in range(8, 40):
            f.write(b">s%07d\n" % i + rows[i].tobytes().lower() + b"\n")
        f.write(b">stranger\n" + b"AG" * 40 + b"\n")
    out = str(tmp_path / "out.tmsa")
    script = os.path.join(REPO, "scripts", "anchor_msa.py")
    r = subprocess.run([sys.executable, script, "-s", seed, "-i", str(queries2), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0 and "Total times" in r.stdout, r.stderr
    assert open(out, "rb").read() == open(original, "rb").read()                    # lower-case input comes out upper-cased
    tsv = open(out + ".anchor.tsv").read().splitlines()
    assert tsv[0].split("\t") == ["id", "status", "score", "d0", "n_match", "n_ins", "n_del", "first_col", "last_col"] and len(tsv) == 34
    assert tsv[1].split("\t")[:5] == [">s0000008", "0", tsv[1].split("\t")[2], "0", tsv[1].split("\t")[4]] and tsv[-1].split("\t")[0] == ">stranger"
    assert int(tsv[-1].split("\t")[1]) & 1 and all(line.split("\t")[1] == "0" for line in tsv[1:-1])
    assert open(out + ".unaligned.fa", "rb").read() == b">stranger\n" + b"AG" * 40 + b"\n"
    r = subprocess.run([sys.executable, script, "-s", seed, "-i", str(queries2), "-o", out, "--no-seed", "--band", "8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == to_fasta(rows[8:], 8)
