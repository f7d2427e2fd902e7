"""Clustering by identity on the device (csrc/cluster.hip behind mp_cluster_load / mp_cluster_pairs / mp_cluster_greedy) against the
yardstick of tests/cluster_ref.py on the cases of tests/cluster_cases.py: the pair records over all ordered pairs and every band form,
the carried-count kernel against the traced one of anchored alignment, the bands on either side of every change of the sweep's lane
form, the LDS sizing at the length limit, the greedy result for every
block size and pair batch, and the script end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import anchor_ref
import cluster_cases as cases
import cluster_ref as ref
from conftest import REPO
from multiprime_amd._abi import ANCHOR_MAX_LEN, MprimeError
from multiprime_amd.cluster import ClusterByIdentity

FIELDS = ("votes", "d0", "score", "n_match", "status")
BANDS = (0, 4, 32, 100, 255)
# 2W + 1 = 63, 127 | 129, 255 | 257 diagonals: the widest band of a lane form (1, 2, 4 diagonals per lane) and the narrowest of the next
EDGE_BANDS = (31, 63, 64, 127, 128)
# twelve records of pair_case() — 8 .. 13, 64, 126, 128 and 172 bases of four families — all ordered pairs aligned (min_votes = 0)
EDGE_RECORDS = (1, 2, 3, 6, 13, 16, 18, 34, 39, 43, 47, 58)
# what the yardstick alone finds among the 144 pairs per band: (paths that touch the band's edge, paths with an indel, status 0)
EDGE_KINDS = {31: (2, 60, 14), 63: (3, 87, 18), 64: (7, 89, 17), 127: (1, 104, 19), 128: (1, 104, 19)}
IDENTITIES = (800, 900, 1000)
SCRIPT = os.path.join(REPO, "scripts", "cluster_by_identity.py")


def pack(seqs):
    raw = [s.encode() for s in seqs]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw), np.uint8), off


@pytest.fixture(scope="module")
def pair_truth():
    """The ~60 records, all ordered pairs (a record against itself included), and the yardstick's record of every pair the default
    min_votes aligns, per band.  A pair without a shared word does not depend on the band."""
    seqs = [s for _, s in cases.pair_case()]
    q, r = np.divmod(np.arange(len(seqs) ** 2), len(seqs))
    want = {W: [ref.pair(seqs[a], seqs[b], band=W, identity_permille=800) for a, b in zip(q, r)] for W in BANDS}
    return seqs, q.astype(np.int32), r.astype(np.int32), want


@pytest.fixture(scope="module")
def edge_truth():
    """EDGE_RECORDS, all ordered pairs, the yardstick's record of every pair per EDGE_BANDS band, and per band how many of the
    alignments hold an indel (ref.pair's records do not keep the gap counts: anchor_ref.align is asked again, as ref.pair asks it)."""
    records = cases.pair_case()
    seqs = [records[k][1] for k in EDGE_RECORDS]
    q, r = np.divmod(np.arange(len(seqs) ** 2), len(seqs))
    want, indels = {}, {}
    for W in EDGE_BANDS:
        want[W] = [ref.pair(seqs[a], seqs[b], band=W, identity_permille=800, min_votes=0) for a, b in zip(q, r)]
        indels[W] = 0
        for a, b, w in zip(q, r, want[W]):
            al = anchor_ref.align(seqs[a].upper(), seqs[b].upper(), list(range(len(seqs[b]))), len(seqs[b]), band=W, min_identity_permille=800, d0=w["d0"])
            assert (al["score"], al["n_match"], al["status"]) == (w["score"], w["n_match"], w["status"])
            indels[W] += al["score"] != ref.NO_SCORE and al["n_ins"] + al["n_del"] > 0
    return seqs, q.astype(np.int32), r.astype(np.int32), want, indels


@pytest.fixture(scope="module")
def greedy_truth():
    """The yardstick's clustering of every case at every identity, computed once (the pair alignments are shared between identities)."""
    out = {}
    for name, records in cases.all_cases().items():
        seqs, memo = [s for _, s in records], {}
        out[name] = {p: ref.cluster(seqs, memo=memo, identity_permille=p) for p in IDENTITIES}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("W", BANDS)
def test_pairs_equal_the_yardstick(W, hip_lib, pair_truth):
    seqs, q, r, want = pair_truth
    assert hip_lib.backend == "hip" and hip_lib.cluster
    ctx = hip_lib.context(0)
    try:
        ctx.cluster_load(*pack(seqs))
        got = ctx.cluster_pairs(q, r, band=W, identity_permille=800).tolist()
        aligned = 0
        for x, (g, w) in enumerate(zip(got, want[W])):
            assert dict(zip(FIELDS, g)) == w, (W, int(q[x]), int(r[x]), g, w)
            aligned += w["status"] != 5
        # 50 of the 60 records hold a 12-mer and words are shared inside a family only: at most 5 * 10 * 10 = 500 ordered pairs can
        # be aligned; the yardstick aligns 334 of them (the substrings of one root need not overlap).  The device aligns those and
        # no other pair.
        assert aligned == 334 and ctx.cluster_stats()[1]["pairs"] == aligned
    finally:
        ctx.close()


@pytest.mark.gpu
def test_pairs_without_a_vote_are_aligned_at_min_votes_0(hip_lib, pair_truth):
    seqs, q, r, _ = pair_truth
    keep = np.flatnonzero((q % 5 == 0) | (r % 7 == 0))
    ctx = hip_lib.context(0)
    try:
        ctx.cluster_load(*pack(seqs))
        got = ctx.cluster_pairs(q[keep], r[keep], band=4, identity_permille=800, min_votes=0).tolist()
        for x, g in zip(keep, got):
            w = ref.pair(seqs[q[x]], seqs[r[x]], band=4, identity_permille=800, min_votes=0)
            assert dict(zip(FIELDS, g)) == w, (int(q[x]), int(r[x]), g, w)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W", BANDS)
def test_carried_counts_equal_the_traced_alignment(W, hip_lib, pair_truth):
    """mp_anchor_align traces its path through stored bits; mp_cluster_pairs carries the counts.  Same pairs, same numbers."""
    seqs, q, r, _ = pair_truth
    n = len(seqs)
    data, off = pack(seqs)
    ctx = hip_lib.context(0)
    try:
        ctx.cluster_load(data, off)
        got = ctx.cluster_pairs(q, r, band=W, identity_permille=800, min_votes=0).reshape(n, n, 5)
        for b in range(n):
            ctx.anchor_set(seqs[b].upper().encode(), np.arange(len(seqs[b])), len(seqs[b]), band=W, min_identity_permille=800)
            _, meta, _ = ctx.anchor_align(data, off)
            for key, col in (("score", 0), ("d0", 1), ("n_match", 2), ("status", 7)):
                assert got[:, b, FIELDS.index(key)].tolist() == meta[:, col].tolist(), (W, b, key)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W", EDGE_BANDS)
def test_bands_at_the_changes_of_the_lane_form(W, hip_lib, edge_truth):
    """The last band of one lane form and the first of the next: the carried counts against the yardstick and against the traced
    alignment, on pairs of which the yardstick says that some touch the band's edge, some hold an indel and some are clean."""
    seqs, q, r, want, indels = edge_truth
    n = len(seqs)
    touched = sum(bool(w["status"] & 2) and w["score"] != ref.NO_SCORE for w in want[W])
    clean = sum(w["status"] == 0 for w in want[W])
    assert (touched, indels[W], clean) == EDGE_KINDS[W] and min(EDGE_KINDS[W]) >= 1
    data, off = pack(seqs)
    ctx = hip_lib.context(0)
    try:
        ctx.cluster_load(data, off)
        got = ctx.cluster_pairs(q, r, band=W, identity_permille=800, min_votes=0)
        for x, (g, w) in enumerate(zip(got.tolist(), want[W])):
            assert dict(zip(FIELDS, g)) == w, (W, int(q[x]), int(r[x]), g, w)
        got = got.reshape(n, n, 5)
        for b in range(n):
            ctx.anchor_set(seqs[b].upper().encode(), np.arange(len(seqs[b])), len(seqs[b]), band=W, min_identity_permille=800)
            _, meta, _ = ctx.anchor_align(data, off)
            for key, col in (("score", 0), ("d0", 1), ("n_match", 2), ("status", 7)):
                assert got[:, b, FIELDS.index(key)].tolist() == meta[:, col].tolist(), (W, b, key)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_two_sequences_at_the_length_limit(hip_lib):
    """Two records of 32767 bases, identical but for substitutions at least 50 bases apart: every substitution is a mismatch of the
    diagonal path (a gap pair around one would cost 24 to save 9), so n_match = m - substitutions."""
    rng = np.random.default_rng(9)
    a = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ANCHOR_MAX_LEN)]
    b = a.copy()
    pos = np.arange(60, ANCHOR_MAX_LEN - 60, 53)
    b[pos] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), a[pos])]
    ctx = hip_lib.context(0)
    try:
        ctx.cluster_load(np.concatenate([a, b]), np.array([0, ANCHOR_MAX_LEN, 2 * ANCHOR_MAX_LEN], np.int64))
        got = ctx.cluster_pairs([1, 0], [0, 1], band=8, identity_permille=950).tolist()
        n_match = ANCHOR_MAX_LEN - len(pos)
        score = 5 * n_match - 4 * len(pos)
        assert got[0][1:] == [0, score, n_match, 0] and got[1][1:] == [0, score, n_match, 0] and got[0][0] > 20000
        cluster_of, reps, nm = ctx.cluster_greedy(band=8, identity_permille=950)
        assert cluster_of.tolist() == [0, 0] and reps.tolist() == [0] and nm.tolist() == [ANCHOR_MAX_LEN, n_match]
    finally:
        ctx.close()


def greedy(hip_lib, seqs, **kw):
    ctx = hip_lib.context(0)
    try:
        ctx.cluster_load(*pack(seqs))
        cluster_of, reps, nm = ctx.cluster_greedy(**kw)
        return cluster_of.tolist(), reps.tolist(), nm.tolist(), ctx.cluster_stats()[1]
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("block", (None, 1, 3, 64))
@pytest.mark.parametrize("name", sorted(cases.all_cases()))
def test_greedy_equals_the_yardstick_for_every_block(name, block, hip_lib, greedy_truth, monkeypatch):
    if block is None:
        monkeypatch.delenv("MP_CLUSTER_BLOCK", raising=False)
    else:
        monkeypatch.setenv("MP_CLUSTER_BLOCK", str(block))
    seqs = [s for _, s in cases.all_cases()[name]]
    for permille in IDENTITIES:
        got = greedy(hip_lib, seqs, identity_permille=permille)
        want = greedy_truth[name][permille]
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2], (name, block, permille)
        if block is not None:
            assert got[3]["rounds"] >= (len(want[1]) + block - 1) // block


@pytest.mark.gpu
def test_greedy_does_not_depend_on_the_pair_batch(hip_lib, greedy_truth, monkeypatch):
    monkeypatch.setenv("MP_CLUSTER_PAIR_BATCH", "7")
    monkeypatch.setenv("MP_CLUSTER_BLOCK", "16")
    seqs = [s for _, s in cases.all_cases()["special"]]
    got = greedy(hip_lib, seqs, identity_permille=800)
    assert got[:3] == tuple(greedy_truth["special"][800])


def run_script(inp, out, *flags):
    return subprocess.run([sys.executable, SCRIPT, "-i", str(inp), "-o", str(out), *flags], capture_output=True, text=True)


@pytest.mark.gpu
def test_the_script_twice_and_the_two_calls_of_the_pipeline(tmp_path, greedy_truth):
    records = cases.all_cases()["special"]
    ids, seqs = [i for i, _ in records], [s for _, s in records]
    inp = tmp_path / "in.fa"
    inp.write_text(cases.fasta(records))
    # -c 1: the duplicate removal; byte-equal to what the yardstick writes, and the same bytes on a second run
    r = run_script(inp, tmp_path / "rmdup.fa", "-c", "1")
    assert r.returncode == 0 and "Total times" in r.stdout, r.stderr
    want = greedy_truth["special"][1000]
    assert (tmp_path / "rmdup.fa.clstr").read_text() == ref.clstr_text(ids, seqs, *want)
    assert (tmp_path / "rmdup.fa").read_text() == ref.rep_fasta(ids, seqs, want[1])
    r = run_script(inp, tmp_path / "again.fa", "-c", "1")
    assert r.returncode == 0, r.stderr
    for tail in ("", ".clstr"):
        assert (tmp_path / ("again.fa" + tail)).read_bytes() == (tmp_path / ("rmdup.fa" + tail)).read_bytes()
    # -c 0.8 on the output of -c 1
    r = run_script(tmp_path / "rmdup.fa", tmp_path / "c80.fa", "-c", "0.8")
    assert r.returncode == 0, r.stderr
    ids2, seqs2 = zip(*ref.read_fasta((tmp_path / "rmdup.fa").read_text()))
    assert list(ids2) == [ids[i] for i in want[1]] and len(ids2) < len(ids)
    want2 = ref.cluster(list(seqs2), identity_permille=800)
    assert (tmp_path / "c80.fa.clstr").read_text() == ref.clstr_text(ids2, seqs2, *want2)
    assert (tmp_path / "c80.fa").read_text() == ref.rep_fasta(ids2, seqs2, want2[1])
    assert len(want2[1]) < len(ids2)


@pytest.mark.gpu
def test_refusals_name_the_record(hip_lib, tmp_path):
    ctx = hip_lib.context(0)
    try:
        with pytest.raises(MprimeError, match="mp_cluster_load first"):
            ctx.cluster_n = 1
            ctx.cluster_greedy()
        data, off = pack(["ACGT" * 5, "AC", "ACGTT"])
        off[2] = off[1]                                             # an empty record: named, nothing launched
        with pytest.raises(MprimeError, match="record 1 has 0 bases"):
            ctx.cluster_load(data, off)
        long = np.full(ANCHOR_MAX_LEN + 1, ord("A"), np.uint8)
        with pytest.raises(MprimeError, match="record 1 has 32768 bases"):
            ctx.cluster_load(np.concatenate([long[:5], long]), np.array([0, 5, 5 + len(long)], np.int64))
        ctx.cluster_load(*pack(["ACGT" * 5, "ACGTT"]))
        with pytest.raises(MprimeError, match="band 256"):
            ctx.cluster_greedy(band=256)
        with pytest.raises(MprimeError, match="score parameter 4096"):
            ctx.cluster_pairs([0], [1], match=4096)
        with pytest.raises(MprimeError, match="pair 0 names sequence 2"):
            ctx.cluster_pairs([2], [1])
    finally:
        ctx.close()
    inp = tmp_path / "long.fa"
    inp.write_text(">ok\nACGTACGTACGTACGT\n>toolong desc\n" + "A" * (ANCHOR_MAX_LEN + 1) + "\n")
    r = run_script(inp, tmp_path / "out.fa")
    assert r.returncode == 1 and ">toolong has 32768 bases" in r.stderr and not (tmp_path / "out.fa").exists()


@pytest.mark.gpu
def test_the_class_and_its_accessors(hip_lib, tmp_path, greedy_truth):
    records = cases.all_cases()["families"]
    inp = tmp_path / "in.fa"
    inp.write_text(cases.fasta(records))
    app = ClusterByIdentity(str(inp), str(tmp_path / "out.fa"), identity=0.9, library=hip_lib).run()
    want = greedy_truth["families"][900]
    assert app.cluster_of().tolist() == want[0] and app.representatives().tolist() == want[1] and app.n_match().tolist() == want[2]
    assert app.ids() == [i for i, _ in records] and app.stats["n_clusters"] == len(want[1]) and app.stats["pairs"] > 0
