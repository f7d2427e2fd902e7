"""Both strands of the identity merge on the device (csrc/ani.hip behind mp_ani_sketch_strands / mp_ani_orientations /
mp_ani_pairs_strand / mp_ani_groups_strand) against the yardstick of tests/ani_strand_ref.py on the cases of tests/ani_cases.py with
records turned: canonical sketches and orientation bits around every size at which the kernel changes its path, the forward
comparison calls on a canonical set, (same, opp) over all ordered pairs, (SAME, OPP) per pair of groups around the tile and chunk
sizes, the refusals, and the script end to end on a tree with two clusters turned."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import ani_cases as cases
import ani_ref as ref
import ani_strand_ref as sref
from anchor_cases import rand_seq
from conftest import REPO
from multiprime_amd._abi import MprimeError

SCRIPT = os.path.join(REPO, "scripts", "merge_cluster_by_ANI.py")


def pack(seqs):
    raw = [s.encode() for s in seqs]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw), np.uint8), off


@pytest.fixture(scope="module")
def sketch_truth():
    """(labels, records, [(hashes, bits)] at a size no record fills): the sketch at size s is the first s of each."""
    recs = cases.sketch_records()
    recs += [("rc of " + label, sref.rc(seq)) for label, seq in recs]          # ("500 x A" gives 500 x T: bit 1 words only)
    x = rand_seq(random.Random(5), 700)
    recs += [("ACGT x 100", "ACGT" * 100), ("x + rc(x)", x + sref.rc(x))]
    return [label for label, _ in recs], [seq for _, seq in recs], [sref.sketch(seq, 1 << 30) for _, seq in recs]


@pytest.mark.gpu
@pytest.mark.parametrize("s", cases.SKETCH_SIZES)
def test_canonical_sketches_and_bits_equal_the_yardstick(s, hip_lib, sketch_truth):
    labels, seqs, full = sketch_truth
    assert hip_lib.backend == "hip" and hip_lib.ani_strands
    ctx = hip_lib.context(0)
    try:
        ctx.ani_sketch(*pack(seqs), s, strands=True)
        hashes, sizes = ctx.ani_sketches()
        bits = ctx.ani_orientations()
        assert bits.shape == (len(seqs), (s + 31) // 32) and bits.dtype == np.uint32
        for label, (want, wbits), row, n, brow in zip(labels, full, hashes, sizes, bits):
            assert n == min(s, len(want)) and row[:n].tolist() == want[:s], (s, label)
            assert (row[n:] == 0xFFFFFFFF).all(), (s, label)
            assert brow.tolist() == sref.bit_words(wbits[:s], s), (s, label)  # (zero past the sketch's size)
        at = labels.index
        assert not bits[at("x + rc(x)")].any() and not bits[at("ACGT x 100")].any() and not bits[at("500 x A")].any()
        assert bits[at("rc of 500 x A")].tolist() == [1] + [0] * ((s + 31) // 32 - 1)
        assert ctx.ani_stats()[1]["sketches"] == len(seqs)
        # a forward set replaces it, and the strand calls refuse that one
        ctx.ani_sketch(*pack(seqs[:4]), s)
        with pytest.raises(MprimeError, match="forward"):
            ctx.ani_orientations()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def turned_pairs():
    """pair_records() with every third record turned, and its canonical yardstick sketches by size (built once per size)."""
    seqs = [sref.rc(x) if i % 3 == 0 else x for i, x in enumerate(cases.pair_records())]
    memo = {}

    def sketches(s):
        if s not in memo:
            memo[s] = [sref.sketch(x, s) for x in seqs]
        return memo[s]
    return seqs, sketches


@pytest.mark.gpu
@pytest.mark.parametrize("s", (16, 100, 1024))
def test_pairs_on_a_canonical_set_equal_the_yardstick(s, hip_lib, turned_pairs):
    seqs, sketches = turned_pairs
    sk = sketches(s)
    a, b = np.divmod(np.arange(len(seqs) ** 2), len(seqs))
    ctx = hip_lib.context(0)
    try:
        ctx.ani_sketch(*pack(seqs), s, strands=True)
        got = ctx.ani_pairs(a, b).tolist()
        for x, g in enumerate(got):
            assert tuple(g) == ref.pair(sk[a[x]][0], sk[b[x]][0], s), (s, int(a[x]), int(b[x]))
        assert got[0 * len(seqs) + 1][2] == 1000000             # record 0 is turned, record 1 is its copy as given
        assert ctx.ani_stats()[1]["pairs"] == len(got)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("s", (16, 100, 1024))
def test_pairs_strand_equals_the_yardstick(s, hip_lib, turned_pairs):
    seqs, sketches = turned_pairs
    sk = sketches(s)
    a, b = np.divmod(np.arange(len(seqs) ** 2), len(seqs))
    ctx = hip_lib.context(0)
    try:
        ctx.ani_sketch(*pack(seqs), s, strands=True)
        got = ctx.ani_pairs_strand(a, b).tolist()
        mixed = minus = 0
        for x, g in enumerate(got):
            p, q = sk[a[x]], sk[b[x]]
            assert tuple(g) == sref.pair_strand(p, q, s), (s, int(a[x]), int(b[x]))
            if not p[0] or not q[0]:
                assert g == [0, 0]
            mixed += (len(p[0]) == s) != (len(q[0]) == s) and sum(g) > 0     # a full sketch against one that is not
            minus += g[1] > g[0]
        assert mixed > 0 and minus > 0
        assert got[0 * len(seqs) + 1][1] > got[0 * len(seqs) + 1][0] and got[1 * len(seqs) + 2][0] > got[1 * len(seqs) + 2][1]
        assert ctx.ani_pairs_strand([], []).shape == (0, 2)
        with pytest.raises(MprimeError, match="names sequence"):
            ctx.ani_pairs_strand([0], [len(seqs)])
        with pytest.raises(MprimeError, match="names sequence"):
            ctx.ani_pairs_strand([-1], [0])
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("turn", ["family", "mixed"])
@pytest.mark.parametrize("s,cap", [(64, None), (1024, None), (64, "3")])
def test_groups_strand_equals_the_yardstick(s, cap, turn, hip_lib, monkeypatch):
    """Every ordered pair of the groups (1, 63, 64, 65 and 500 members among them) at three floors, with the second family turned
    (its members still agree with each other: every vote is +) and with the third family and record 3, the one member of the first
    group, turned (that group votes - against its own family).  The
    yardstick's (ani_ppm, same, opp) of every pair of the 24 distinct records is computed once; a group pair's numbers are sums over
    the members' records.  cap: MP_ANI_MAX_GRID, which cuts the workgroups of a group pair over several launches."""
    records, groups = cases.group_records()
    records = [sref.rc(x) if (7 <= i < 14 if turn == "family" else i == 3 or 14 <= i < 21) else x for i, x in enumerate(records)]
    sk = [sref.sketch(x, s) for x in records]
    ani = np.array([[ref.pair(p[0], r[0], s)[2] for r in sk] for p in sk], np.int64)
    vote = np.array([[sref.pair_strand(p, r, s) for r in sk] for p in sk], np.int64)
    seqs = [records[i] for g in groups for i in g]
    group_off = np.cumsum([0] + [len(g) for g in groups])
    q, r = np.divmod(np.arange(len(groups) ** 2), len(groups))
    if cap:
        monkeypatch.setenv("MP_ANI_MAX_GRID", cap)
    ctx = hip_lib.context(0)
    try:
        ctx.ani_sketch(*pack(seqs), s, strands=True)
        signs = set()
        for floor in (0, 700000, 1000000):
            got = ctx.ani_groups_strand(group_off, q, r, floor).tolist()
            numbers = ctx.ani_groups(group_off, q, r, floor).tolist()
            for x, g in enumerate(got):
                ix = np.ix_(groups[q[x]], groups[r[x]])
                m = ani[ix] >= floor
                assert g == [int(vote[ix][..., 0][m].sum()), int(vote[ix][..., 1][m].sum())], (s, floor, int(q[x]), int(r[x]))
                assert numbers[x][0] == int(m.sum())
                if numbers[x][0] == 0:
                    assert g == [0, 0]
                signs.add(sref.strand(*g))
        assert signs == ({"+"} if turn == "family" else {"+", "-"})
        small = sref.groups_strand([sk[i] for i in groups[0]], [sk[i] for i in groups[1]], s, 700000)
        assert tuple(ctx.ani_groups_strand(group_off, [0], [1], 700000)[0]) == small and sum(small) > 0
        with pytest.raises(MprimeError, match="group"):
            ctx.ani_groups_strand(group_off, [0], [len(groups)], 700000)
        with pytest.raises(MprimeError, match="report_ppm"):
            ctx.ani_groups_strand(group_off, [0], [1], 1000001)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_strand_calls_refuse_a_forward_set(hip_lib):
    seqs = cases.pair_records()[:12]
    ctx = hip_lib.context(0)
    try:
        for call in (ctx.ani_orientations, lambda: ctx.ani_pairs_strand([0], [1]), lambda: ctx.ani_groups_strand([0, 6, 12], [0], [1])):
            with pytest.raises(MprimeError, match="mp_ani_sketch_strands first") as e:
                call()
            assert e.value.code == -1
        ctx.ani_sketch(*pack(seqs), 100)
        for call in (ctx.ani_orientations, lambda: ctx.ani_pairs_strand([0], [1]), lambda: ctx.ani_groups_strand([0, 6, 12], [0], [1])):
            with pytest.raises(MprimeError, match="forward") as e:
                call()
            assert e.value.code == -1                           # MP_ERR_ARG
        assert tuple(ctx.ani_pairs([1], [2])[0]) == ref.pair(ref.sketch(seqs[1], 100), ref.sketch(seqs[2], 100), 100)      # the forward set serves on
        ctx.ani_sketch(*pack(seqs), 100, strands=True)
        a, b = sref.sketch(seqs[1], 100), sref.sketch(seqs[2], 100)
        assert tuple(ctx.ani_pairs_strand([1], [2])[0]) == sref.pair_strand(a, b, 100)
        for bad in (lambda: ctx.ani_sketch(*pack(["ACGT" * 8192]), 100, strands=True), lambda: ctx.ani_sketch(*pack(seqs), 8, strands=True)):
            with pytest.raises(MprimeError):
                bad()
            assert tuple(ctx.ani_pairs_strand([1], [2])[0]) == sref.pair_strand(a, b, 100)       # a refused call keeps the resident set
    finally:
        ctx.close()


# ---- the script --------------------------------------------------------------------------------------------------------------------------
def run_script(root, *flags):
    res = subprocess.run([sys.executable, SCRIPT, "-i", "cluster.txt", "-p", "20", "-t", "20", "-o", "history.txt", "-a", "0.8"] + list(flags),
                         cwd=root, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    return ref.snapshot(root)


def forward_yardstick(root, drop):
    """ani_ref's decision and file operations on the tree at root, in place; returns the history text."""
    clusters = ref.parse_clusters(open(os.path.join(root, "cluster.txt")).read())
    numbers = ref.tree_numbers(clusters, os.path.join(root, "Clusters_fa"), 1024, 700000)
    md = ref.merge_dict(clusters, "Clusters_fa", ref.decide(clusters, 20, 800000, numbers))
    open(os.path.join(root, "history.txt"), "w").write(ref.history_text(md))
    ref.apply(clusters, os.path.join(root, "Clusters_fa"), {os.path.join(root, k): [os.path.join(root, x) for x in v] for k, v in md.items()}, drop)
    return ref.history_text(md)


@pytest.mark.gpu
def test_script_on_a_tree_with_turned_clusters(hip_lib, tmp_path):
    """semantics_clusters() with the records of Q and U turned: R <- Q <- P is a chain only on both strands."""
    given = cases.semantics_clusters()
    turned = {k: [(i, sref.rc(s)) for i, s in v] if k in ("Q", "U") else v for k, v in given.items()}
    roots = {}
    for name, named in (("unturned", given), ("forward", turned), ("plain", turned), ("both", turned), ("orient", turned)):
        roots[name] = str(tmp_path / name)
        os.makedirs(roots[name])
        cases.write_tree(roots[name], named)
    fresh = ref.snapshot(roots["plain"])
    chain = "Clusters_fa/Q_4\tClusters_fa/P_2\nClusters_fa/R_8\tClusters_fa/Q_4\n"
    assert forward_yardstick(roots["unturned"], "F") == chain
    # without the flags the Q merges are missed, and every output is the forward rule's, byte for byte
    missed = forward_yardstick(roots["forward"], "F")
    assert "Q_4" not in missed
    plain = run_script(roots["plain"], "-d", "F")
    assert plain == ref.snapshot(roots["forward"]) and "history.txt.strand" not in plain
    # both strands: the history of the unturned tree, a strand per line, and the files appended as they are
    both = run_script(roots["both"], "-d", "F", "--both-strands")
    assert both["history.txt"].decode() == chain
    lines = [x.split("\t") for x in both["history.txt.strand"].decode().splitlines()]
    assert [x[:3] for x in lines] == [["Clusters_fa/Q_4", "Clusters_fa/P_2", "-"], ["Clusters_fa/R_8", "Clusters_fa/Q_4", "-"]]
    sk = {k: [sref.sketch(s, 1024) for _, s in v] for k, v in turned.items() if k in "PQR"}
    assert [tuple(int(v) for v in x[3:]) for x in lines] == [sref.groups_strand(sk["P"], sk["Q"], 1024, 700000), sref.groups_strand(sk["Q"], sk["R"], 1024, 700000)]
    for ext in (".fa", ".tfa", ".txt"):
        assert both["Clusters_fa/R_14" + ext] == b"".join(fresh["Clusters_fa/%s%s" % (x, ext)] for x in ("R_8", "Q_4", "P_2"))
    # orient: the receiving file has one orientation — every record is reported against R's first record by the forward rule
    orient = run_script(roots["orient"], "-d", "F", "--both-strands", "--orient")
    assert orient["history.txt"] == both["history.txt"] and orient["history.txt.strand"] == both["history.txt.strand"]
    assert orient["Clusters_fa/R_14.txt"] == both["Clusters_fa/R_14.txt"]
    for ext in (".fa", ".tfa"):
        recs = ref.read_fasta(os.path.join(roots["orient"], "Clusters_fa", "R_14" + ext))
        assert recs == given["R"] + given["Q"] + given["P"]    # P was turned twice
        first = ref.sketch(recs[0][1], 1024)
        assert all(ref.pair(ref.sketch(seq, 1024), first, 1024)[2] >= 700000 for _, seq in recs)
    mixed = ref.read_fasta(os.path.join(roots["both"], "Clusters_fa", "R_14.tfa"))
    first = ref.sketch(mixed[0][1], 1024)
    assert [ref.pair(ref.sketch(seq, 1024), first, 1024)[2] >= 700000 for _, seq in mixed] == [True] * 8 + [False] * 4 + [True] * 2
    assert {k: v for k, v in orient.items() if "R_14" not in k} == {k: v for k, v in both.items() if "R_14" not in k}
