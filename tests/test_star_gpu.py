"""The star alignment on the device (csrc/star.hip behind mp_star_load / mp_star_round) against the yardstick of tests/star_ref.py on
the cases of tests/star_cases.py: every round's rows byte for byte, meta, ins, counts, width and the anchor the counts lead to must be
equal.  Then the batching, the refusals, the drop-in end to end, and the reference workflow's own 500-record cluster."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import star_cases as cases
import star_ref as ref
from anchor_ref import align as ref_align, anchor_of
from conftest import GOLDEN, REPO, golden_input
from multiprime_amd._abi import MprimeError
from multiprime_amd.starmsa import StarAlignment, anchor_of_counts

FIELDS = ("score", "d0", "n_match", "n_ins", "n_del", "first_col", "last_col", "status")


@pytest.fixture(scope="module")
def truth():
    """The yardstick's results of every group, computed once."""
    groups = cases.all_groups()
    return groups, [cases.yardstick(g) for g in groups]


def pack(records):
    raw = [q.encode() for q in records]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw), np.uint8), off


def device_round(ctx, anchor, params):
    """One round as the yardstick's dict, plus the anchor its counts lead to."""
    meta, ins, width = ctx.star_round(anchor.encode(), **params)
    rows, counts = ctx.star_rows(), ctx.star_counts()
    placed = (meta[:, 7] & 1) == 0
    assert rows.shape == (len(meta), width) and counts.shape == (width, 6) and ctx.star_stats()[1]["placed"] == placed.sum()
    assert all(set(r.tobytes()) == {ord("-")} for r in rows[~placed])
    return dict(rows=[r.tobytes().decode() if ok else None for r, ok in zip(rows, placed)],
                meta=[dict(zip(FIELDS + ("band",), mt[:8] + [mt[10]])) for mt in meta.tolist()], ins=ins.tolist(), width=width,
                counts=counts.tolist(), placed=placed.tolist(), next_anchor=anchor_of_counts(counts, int(placed.sum())).decode())


def same_round(got, want, what):
    for key in ("width", "ins", "placed", "counts"):
        assert got[key] == want[key], (what, key)
    for q, (a, b) in enumerate(zip(got["meta"], want["meta"])):
        assert a == b, (what, q, a, b)
    assert got["rows"] == want["rows"], what
    kept = [r for r in want["rows"] if r is not None]
    assert got["next_anchor"] == anchor_of(kept)[0], what


def same_group(ctx, g, want):
    ctx.star_load(*pack(cases.cleaned(g)))
    for k, (anchor, rnd) in enumerate(zip(want["anchors"], want["rounds"])):
        got = device_round(ctx, anchor, g["params"])
        same_round(got, rnd, (g["name"], k))
        if k + 1 < len(want["anchors"]):
            assert got["next_anchor"] == want["anchors"][k + 1]
        elif k + 1 < g["rounds"]:
            assert got["next_anchor"] == anchor           # the yardstick stopped early: so would the device's counts


@pytest.mark.gpu
def test_every_group_equals_the_yardstick(hip_lib, truth):
    assert hip_lib.backend == "hip" and hip_lib.star
    ctx = hip_lib.context(0)
    try:
        for g, want in zip(*truth):
            same_group(ctx, g, want)
        names = [g["name"] for g in truth[0]]
        # n + 1 and L' no multiples of 16; a run of 40 inserted bases; bands 64 and 255
        g, want = truth[0][names.index("slot0-slotn")], truth[1][names.index("slot0-slotn")]
        assert (len(want["anchors"][0]) + 1) % 16 and want["rounds"][0]["width"] % 16
        assert max(truth[1][names.index("drift-64-ins")]["rounds"][0]["ins"]) == 40
        assert truth[1][names.index("drift-255")]["rounds"][0]["meta"][1]["band"] == 255
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def batch_truth():
    g = cases.batch_group()
    sub = dict(g, records=g["records"][:65])
    return g, sub, cases.yardstick(sub)


@pytest.mark.gpu
@pytest.mark.parametrize("n_records", (1, 63, 64, 65, 200))
def test_results_do_not_depend_on_the_batch(n_records, hip_lib, batch_truth, monkeypatch):
    g, sub, want = batch_truth
    records = g["records"][:n_records]
    ctx = hip_lib.context(0)
    try:
        ctx.star_load(*pack(records))
        out = []
        for cap in ("64", None):
            if cap:
                monkeypatch.setenv("MP_STAR_BATCH", cap)
            else:
                monkeypatch.delenv("MP_STAR_BATCH")
            anchor, rounds = records[0], []
            for _ in range(2):
                rounds.append(device_round(ctx, anchor, g["params"]))
                stats = ctx.star_stats()[1]
                assert stats["batches"] == ((n_records + 63) // 64 if cap else 1)
                levels = {32: 0, 64: 1, 128: 2, 255: 3}
                assert stats["realigned"] == sum(levels[m["band"]] for m in rounds[-1]["meta"])
                if len(rounds) == 1:                      # against the planted anchor every tenth record drifts
                    assert stats["realigned"] == len(range(3, n_records, 10))
                anchor = rounds[-1]["next_anchor"]
            out.append(rounds)
        assert out[0] == out[1]
        if n_records == 65:
            for k, rnd in enumerate(want["rounds"]):
                same_round(out[0][k], rnd, ("batch", k))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_refusals(hip_lib):
    ctx = hip_lib.context(0)
    try:
        with pytest.raises(MprimeError, match="no records"):
            ctx.star_round(b"ACGT")
        data, off = pack(["ACGT", "AC"])
        off[2] = off[1]                                             # an empty record: named, nothing launched
        with pytest.raises(MprimeError, match="record 1"):
            ctx.star_load(data, off)
        with pytest.raises(MprimeError, match="record 0"):
            ctx.star_load(*pack(["A" * 32768]))
        with pytest.raises(MprimeError, match="no round"):
            ctx.star_load(*pack(["ACGT"]))
            ctx.star_rows()
        with pytest.raises(MprimeError, match="band"):
            ctx.star_round(b"ACGT", band=0)
        ctx.star_free()
        with pytest.raises(MprimeError, match="no records"):
            ctx.star_round(b"ACGT")
    finally:
        ctx.close()


def _fasta(path, g, ids=None):
    with open(path, "w") as f:
        for q, r in enumerate(g["records"]):
            f.write(f">{ids[q] if ids else 'r%03d' % q} some description\n{r}\n")


@pytest.mark.gpu
def test_the_class(hip_lib, truth, tmp_path):
    for name in ("consensus-moves", "consensus-stays", "gapped-input", "single"):
        g, want = next((g, w) for g, w in zip(*truth) if g["name"] == name)
        inp, out = str(tmp_path / (name + ".fa")), str(tmp_path / (name + ".tmsa"))
        _fasta(inp, g)
        p = g["params"]
        app = StarAlignment(inp, out, rounds=g["rounds"], band=p["band"], match=p["match"], mismatch=p["mismatch"], gap_open=p["gap_open"],
                            gap_extend=p["gap_extend"], min_identity=p["min_identity_permille"] / 1000, library=hip_lib).run()
        assert [a.decode() for a in app.anchors()] == want["anchors"] and app.stats["rounds"] == len(want["anchors"])
        last = want["rounds"][-1]
        assert [r.tobytes().decode() for r in app.rows()] == [r if r is not None else "-" * last["width"] for r in last["rows"]]
        assert [m["band"] for m in app.meta()] == [m["band"] for m in last["meta"]] and app.ins().tolist() == last["ins"]
        assert app.ids() == [">r%03d" % q for q in range(len(g["records"]))]
        lines = open(out).read().splitlines()
        assert lines[0::2] == [i for i, r in zip(app.ids(), last["rows"]) if r is not None] and lines[1::2] == [r for r in last["rows"] if r is not None]


@pytest.mark.gpu
def test_the_script(hip_lib, truth, tmp_path):
    g, want = next((g, w) for g, w in zip(*truth) if g["name"] == "unplaced")
    inp, out = str(tmp_path / "in.tfa"), str(tmp_path / "out.tmsa")
    _fasta(inp, g, ids=["a", "b", "stranger", "d"])
    script = os.path.join(REPO, "scripts", "run_mafft.py")
    r = subprocess.run([sys.executable, script, "-i", inp, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0 and "Total times" in r.stdout, r.stderr
    last = want["rounds"][-1]
    assert open(out).read().splitlines() == [x for i, row in zip((">a", ">b", ">stranger", ">d"), last["rows"]) if row is not None for x in (i, row)]
    tsv = open(out + ".star.tsv").read().splitlines()
    assert tsv[0].split("\t") == ["id", "status", "band", "score", "d0", "n_match", "n_ins", "n_del"] and len(tsv) == 5 + len(want["rounds"])
    for line, i, m in zip(tsv[1:5], (">a", ">b", ">stranger", ">d"), last["meta"]):
        assert line.split("\t") == [i] + [str(m[k]) for k in ("status", "band", "score", "d0", "n_match", "n_ins", "n_del")]
    assert tsv[-1] == "# round {}: n {} width {} placed 3 band_warnings {}".format(len(want["rounds"]) - 1, len(want["anchors"][-1]), last["width"],
                                                                                  sum(1 for m in last["meta"] if m["status"] & 2))
    assert open(out + ".unaligned.fa").read() == ">stranger\n" + g["records"][2] + "\n"
    # the core step reads the file: the device's answer equals the CPU checker's on the same file
    from test_anchor_gpu import _core
    from multiprime_amd._abi import Library
    ora = Library(os.path.join(REPO, "oracle", "_build", "libmprime_oracle.so"))
    fam, fam_want = next((g, w) for g, w in zip(*truth) if g["name"] == "family1")
    inp2, out2 = str(tmp_path / "family.tfa"), str(tmp_path / "family.tmsa")
    _fasta(inp2, fam)
    r = subprocess.run([sys.executable, script, "-i", inp2, "-o", out2, "--rounds", "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out2).read().splitlines()[1::2] == fam_want["rounds"][0]["rows"]
    tsv = _core(hip_lib, out2, str(tmp_path / "hip.tsv"))
    assert tsv == _core(ora, out2, str(tmp_path / "ora.tsv")) and tsv.count(b"\n") > 1
    # exit statuses: bad flags 2; an unreadable input, an empty input, a refused record 1
    run = lambda *a: subprocess.run([sys.executable, script] + list(a), capture_output=True, text=True)      # noqa: E731
    assert run("-i", inp, "-o", out, "--rounds", "9").returncode == 2 and run("-i", inp, "-o", out, "--band", "0").returncode == 2
    assert run("-i", str(tmp_path / "missing.fa"), "-o", out).returncode == 1
    empty, refused = tmp_path / "empty.fa", tmp_path / "refused.fa"
    empty.write_text("")
    refused.write_text(">x\nACGT\n>gaps\n--..\n")
    assert run("-i", str(empty), "-o", out).returncode == 1
    r = run("-i", str(refused), "-o", out)
    assert r.returncode == 1 and ">gaps" in r.stderr


def _fasta_records(raw):
    ids, seqs = [], []
    for line in raw.decode().splitlines():
        if line.startswith(">"):
            ids.append(line.split()[0])
            seqs.append("")
        elif line.strip():
            seqs[-1] += line.strip()
    return ids, seqs


def _pairs_share(rows_a, rows_b, fixed):
    """Share of the residue pairs aligned in rows_a (between every row and the rows `fixed`) that are aligned in rows_b too."""
    def residue_index(rows):
        arr = np.array([np.frombuffer(r.encode(), np.uint8) for r in rows])
        letter = arr != ord("-")
        return letter, np.cumsum(letter, axis=1) - 1
    la, ia = residue_index(rows_a)
    lb, ib = residue_index(rows_b)
    n_rows = len(rows_a)
    # column of residue k of row r in b
    colb = [np.flatnonzero(lb[r]) for r in range(n_rows)]
    hit = total = 0
    for f in fixed:
        for r in range(n_rows):
            if r == f:
                continue
            both = la[r] & la[f]
            kr, kf = ia[r][both], ia[f][both]
            total += len(kr)
            hit += int((colb[r][kr] == colb[f][kf]).sum())
    return hit / max(total, 1)


def _majority_share(rows):
    arr = np.array([np.frombuffer(r.encode(), np.uint8) for r in rows])
    letters = arr != ord("-")
    cols = 2 * letters.sum(axis=0) > len(rows)
    best = np.max([(arr == ord(b)).sum(axis=0) for b in "ACGT"], axis=0)
    return float((best[cols] / letters.sum(axis=0)[cols]).mean()), int(cols.sum())


@pytest.mark.gpu
def test_the_reference_cluster(hip_lib, tmp_path):
    """The workflow's own Cluster_0_20727 (500 records of 1698..1867 bases).  Gated: lossless rows of one width, and three fixed records
    equal the yardstick against the device's final anchor.  Printed, not gated (nobody has measured them before): agreement with mafft's
    alignment of the same records and the core step's output on both."""
    inp, out = str(tmp_path / "Cluster_0_20727.tfa"), str(tmp_path / "Cluster_0_20727.tmsa")
    with open(inp, "wb") as f:
        f.write(golden_input("Cluster_0_20727.tfa"))
    ids, seqs = _fasta_records(golden_input("Cluster_0_20727.tfa"))
    mids, mrows = _fasta_records(golden_input("Cluster_0_20727.tmsa"))
    mafft = dict(zip(mids, (r.upper() for r in mrows)))
    assert len(ids) == 500 and sorted(ids) == sorted(mids)
    fixed = list(range(0, 500, 64))                                   # 8 fixed rows
    print()
    for rounds in (1, 2, 3):
        app = StarAlignment(inp, out, rounds=rounds, library=hip_lib).run()
        rows = [r.tobytes().decode() for r in app.rows()]
        meta = app.meta()
        placed = [not m["status"] & 1 for m in meta]
        assert app.ids() == ids and len({len(r) for r in rows}) == 1
        assert all(r.replace("-", "") == s.upper() for r, s, ok in zip(rows, seqs, placed) if ok) and sum(placed) >= 1
        keep = [q for q in range(500) if placed[q]]
        share = _pairs_share([mafft[ids[q]] for q in keep], [rows[q] for q in keep], [keep.index(f) for f in fixed if f in keep])
        ours, n_cols = _majority_share([rows[q] for q in keep])
        theirs, m_cols = _majority_share([mafft[i] for i in ids])
        st = app.round_stats[-1]
        print(f"star rounds={rounds} (ran {len(app.anchors())}): width {len(rows[0])} placed {sum(placed)} band>32 {sum(m['band'] > 32 for m in meta)} "
              f"touched {sum(bool(m['status'] & 2) for m in meta)} anchor n {st['n']}; mafft pairs kept {share:.4f}; majority-letter share "
              f"{ours:.4f} over {n_cols} columns (mafft {theirs:.4f} over {m_cols}); device ms " +
              " ".join(f"{k[:-3]} {st[k]:.2f}" for k in ("vote_ms", "dp_ms", "trace_ms", "profile_ms", "write_ms", "count_ms", "call_ms")))
        if rounds == 2:
            final, anchor = app, app.anchors()[-1].decode()
            n = len(anchor)
            for q in (0, 250, 499):
                want, W = ref.align_escalating(seqs[q].upper(), anchor, 32, match=5, mismatch=4, gap_open=10, gap_extend=2, min_identity_permille=500)
                got = meta[q]
                assert [got[k] for k in FIELDS] + [got["band"]] == [want[k] for k in FIELDS] + [W], q
                # the whole row, rebuilt from the yardstick's path and the device's ins (steps 5 and 6 of the rule)
                assert placed[q], q
                runs, pairs = ref.runs_of(want)
                ins = final.ins().tolist()
                acol = (np.arange(n + 1) + np.cumsum(ins)).tolist()
                assert len(ins) == n + 1 and acol[n] == len(rows[q]) and all(ins[j] >= length for j, (_, length) in runs.items()), q
                row, rec = ["-"] * acol[n], seqs[q].upper()
                for i, j in pairs:
                    row[acol[j]] = rec[i]
                for j, (start, length) in runs.items():
                    at = acol[j] - ins[j] + (ins[j] - length if start == 0 else 0)
                    row[at:at + length] = rec[start:start + length]
                assert rows[q] == "".join(row), q
            from test_anchor_gpu import _core
            tsv = _core(hip_lib, out, str(tmp_path / "star.tsv")).decode().splitlines()
            gold = open(os.path.join(GOLDEN, "cluster0_v1.tsv")).read().splitlines()
            best = lambda t: max((int(x.split("\t")[6]) for x in t[1:]), default=0)       # noqa: E731
            print(f"core step (l 18, f 0.8 here / cluster0_v1 on mafft's rows): {len(tsv) - 1} rows, best coverage {best(tsv)} / {len(gold) - 1} rows, best coverage {best(gold)}")
