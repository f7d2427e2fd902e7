"""The identity merge on the device (csrc/ani.hip behind mp_ani_sketch / mp_ani_pairs / mp_ani_groups) against the yardstick of
tests/ani_ref.py on the cases of tests/ani_cases.py: sketches hash for hash around every size at which the kernel changes its path,
(w, u, ani_ppm) over all ordered pairs, (n_rep, sum_ppm) per pair of groups around the tile and chunk sizes, the device pass for every
ref block size, the script end to end and its refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ani_cases as cases
import ani_ref as ref
from conftest import REPO, load_gz_json
from multiprime_amd._abi import MprimeError
from multiprime_amd.animerge import merge_clstr

SCRIPT = os.path.join(REPO, "scripts", "merge_cluster_by_ANI.py")


def pack(seqs):
    raw = [s.encode() for s in seqs]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw), np.uint8), off


@pytest.fixture(scope="module")
def sketch_truth():
    """Every distinct hash of every record of the sketch case, ascending: the sketch at size s is its first s entries."""
    recs = cases.sketch_records()
    return [label for label, _ in recs], [seq for _, seq in recs], [ref.sketch(seq, 1 << 30) for _, seq in recs]


@pytest.mark.gpu
@pytest.mark.parametrize("s", cases.SKETCH_SIZES)
def test_sketches_equal_the_yardstick(s, hip_lib, sketch_truth):
    labels, seqs, full = sketch_truth
    assert hip_lib.backend == "hip" and hip_lib.ani
    ctx = hip_lib.context(0)
    try:
        ctx.ani_sketch(*pack(seqs), s)
        hashes, sizes = ctx.ani_sketches()
        for label, want, row, n in zip(labels, full, hashes, sizes):
            assert n == min(s, len(want)) and row[:n].tolist() == want[:s], (s, label)
            assert (row[n:] == 0xFFFFFFFF).all(), (s, label)
        assert ctx.ani_stats()[1]["sketches"] == len(seqs)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("s", (16, 100, 1024))
def test_pairs_equal_the_yardstick(s, hip_lib):
    seqs = cases.pair_records()
    sk = [ref.sketch(x, s) for x in seqs]
    a, b = np.divmod(np.arange(len(seqs) ** 2), len(seqs))
    ctx = hip_lib.context(0)
    try:
        ctx.ani_sketch(*pack(seqs), s)
        got = ctx.ani_pairs(a, b).tolist()
        for x, g in enumerate(got):
            assert tuple(g) == ref.pair(sk[a[x]], sk[b[x]], s), (s, int(a[x]), int(b[x]))
        assert ctx.ani_stats()[1]["pairs"] == len(got)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("s", (64, 1024))
def test_groups_equal_the_yardstick(s, hip_lib):
    """Every ordered pair of the groups (q = r included) at three floors.  The yardstick's ani_ppm of every pair of the 24 distinct
    records is computed once; a group pair's numbers are its sum over the members' records."""
    records, groups = cases.group_records()
    sk = [ref.sketch(x, s) for x in records]
    ani = np.array([[ref.pair(p, r, s)[2] for r in sk] for p in sk], np.int64)
    seqs = [records[i] for g in groups for i in g]
    group_off = np.cumsum([0] + [len(g) for g in groups])
    q, r = np.divmod(np.arange(len(groups) ** 2), len(groups))
    ctx = hip_lib.context(0)
    try:
        ctx.ani_sketch(*pack(seqs), s)
        for floor in (0, 700000, 1000000):
            got = ctx.ani_groups(group_off, q, r, floor).tolist()
            for x, g in enumerate(got):
                m = ani[np.ix_(groups[q[x]], groups[r[x]])]
                assert g == [int((m >= floor).sum()), int(m[m >= floor].sum())], (s, floor, int(q[x]), int(r[x]))
            if floor == 700000:
                assert got[0 * len(groups) + 6] == [0, 0] and got[4 * len(groups) + 4][0] > 0
        small = ref.groups([sk[i] for i in groups[0]], [sk[i] for i in groups[1]], s, 700000)
        assert tuple(ctx.ani_groups(group_off, [0], [1], 700000)[0]) == small
        with pytest.raises(MprimeError, match="group"):
            ctx.ani_groups(group_off, [0], [len(groups)], 700000)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", ["1", "7"])
def test_work_split_over_several_launches(cap, hip_lib, monkeypatch):
    """A launch holds fewer than 2^32 work-items, so a large call goes out as several launches that add into the same outputs.
    MP_ANI_MAX_GRID lowers the cap to 1 and 7 workgroups: the sketch lists, the pair batches and the group pairs' workgroups (up to 504
    for 500 x 500 records) are all cut many times, in the middle of a group pair too, and nothing changes."""
    records, groups = cases.group_records()
    s = 64
    sk = [ref.sketch(x, s) for x in records]
    ani = np.array([[ref.pair(p, r, s)[2] for r in sk] for p in sk], np.int64)
    member = [i for g in groups for i in g]
    group_off = np.cumsum([0] + [len(g) for g in groups])
    q, r = np.divmod(np.arange(len(groups) ** 2), len(groups))
    a, b = np.arange(301) % len(member), (np.arange(301) * 37) % len(member)
    monkeypatch.setenv("MP_ANI_MAX_GRID", cap)
    ctx = hip_lib.context(0)
    try:
        ctx.ani_sketch(*pack([records[i] for i in member]), s)
        hashes, sizes = ctx.ani_sketches()
        for x, i in enumerate(member):
            assert hashes[x, :sizes[x]].tolist() == sk[i] and sizes[x] == len(sk[i]), (cap, x)
        for x, g in enumerate(ctx.ani_pairs(a, b).tolist()):
            assert tuple(g) == ref.pair(sk[member[a[x]]], sk[member[b[x]]], s), (cap, x)
        for x, g in enumerate(ctx.ani_groups(group_off, q, r, 700000).tolist()):
            m = ani[np.ix_(groups[q[x]], groups[r[x]])]
            assert g == [int((m >= 700000).sum()), int(m[m >= 700000].sum())], (cap, int(q[x]), int(r[x]))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_a_refused_sketch_call_keeps_the_resident_set(hip_lib):
    seqs = cases.pair_records()[:12]
    ctx = hip_lib.context(0)
    try:
        ctx.ani_sketch(*pack(seqs), 100)
        before = ctx.ani_sketches()
        for bad in (lambda: ctx.ani_sketch(*pack(["ACGT" * 8192]), 100), lambda: ctx.ani_sketch(*pack(seqs), 8)):
            with pytest.raises(MprimeError):
                bad()
            after = ctx.ani_sketches()
            assert after[0].shape == (12, 100) and (after[0] == before[0]).all() and (after[1] == before[1]).all()
        assert tuple(ctx.ani_pairs([1], [2])[0]) == ref.pair(ref.sketch(seqs[1], 100), ref.sketch(seqs[2], 100), 100)
    finally:
        ctx.close()


# ---- the device pass and the script ---------------------------------------------------------------------------------------------------------
def trees():
    golden = load_gz_json("ani_small.json.gz")
    return {"golden": ({k: (None if v is None else v.encode()) for k, v in golden["input"].items()}, golden["meta"]["t"], 0.7),
            "chain": (None, 20, 0.8)}


def plant(root, name):
    snap, t, a = trees()[name]
    if snap is None:
        cases.write_tree(root, cases.semantics_clusters())
    else:
        ref.restore(root, snap)
    return t, a


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["golden", "chain"])
def test_device_pass_for_every_ref_block(name, hip_lib, tmp_path, monkeypatch):
    t, a = plant(str(tmp_path), name)
    monkeypatch.chdir(tmp_path)
    clusters = ref.parse_clusters(open("cluster.txt").read())
    numbers = ref.tree_numbers(clusters, "Clusters_fa", 1024, 700000)
    want = ref.merge_dict(clusters, "Clusters_fa", ref.decide(clusters, t, int(round(a * 1e6)), numbers))
    assert want
    seen = []
    for block in ("1", "3", None):
        if block is None:
            monkeypatch.delenv("MP_ANI_REF_BLOCK", raising=False)
        else:
            monkeypatch.setenv("MP_ANI_REF_BLOCK", block)
        app = merge_clstr(inputfile="cluster.txt", output="history.txt", threshold=t, drop="T", ani=a, library=hip_lib)
        app.load()
        got = app.compare()
        assert got and all(v == numbers(p, r) for (p, r), v in got.items()), block
        assert app.decide(got) == want, block
        assert app.stats["pairs"] > 0 and app.stats["sketches"] == sum(n for _, n in clusters)
        seen.append(len(got))
    assert seen[0] <= seen[1] <= seen[2]       # a smaller block drops a decided cluster sooner


@pytest.mark.gpu
@pytest.mark.parametrize("name,drop", [("golden", "T"), ("golden", "F"), ("chain", "T"), ("chain", "F")])
def test_script_end_to_end(name, drop, hip_lib, tmp_path):
    """The files equal the yardstick's (for the golden tree: the reference's), and a second run from a fresh copy writes the same bytes."""
    runs = []
    for run in ("want", "one", "two"):
        root = str(tmp_path / run)
        os.makedirs(root)
        t, a = plant(root, name)
        if run == "want":
            clusters = ref.parse_clusters(open(os.path.join(root, "cluster.txt")).read())
            numbers = ref.tree_numbers(clusters, os.path.join(root, "Clusters_fa"), 1024, 700000)
            md = ref.merge_dict(clusters, "Clusters_fa", ref.decide(clusters, t, int(round(a * 1e6)), numbers))
            open(os.path.join(root, "history.txt"), "w").write(ref.history_text(md))
            ref.apply(clusters, os.path.join(root, "Clusters_fa"), {os.path.join(root, k): [os.path.join(root, x) for x in v] for k, v in md.items()}, drop)
        else:
            res = subprocess.run([sys.executable, SCRIPT, "-i", "cluster.txt", "-p", "20", "-t", str(t), "-o", "history.txt", "-d", drop, "-a", str(a)],
                                 cwd=root, capture_output=True, text=True, timeout=300)
            assert res.returncode == 0, res.stderr
            assert "Total times" in res.stdout
        runs.append(ref.snapshot(root))
    assert runs[0] == runs[1] == runs[2]
    if name == "golden":
        golden = load_gz_json("ani_small.json.gz")
        assert runs[1] == {k: (None if v is None else v.encode()) for k, v in golden[drop].items()}


@pytest.mark.gpu
def test_refusals_leave_the_tree_untouched(hip_lib, tmp_path):
    root = str(tmp_path)
    plant(root, "golden")
    before = ref.snapshot(root)

    def run(*extra):
        return subprocess.run([sys.executable, SCRIPT, "-i", "cluster.txt", "-t", "3", "-o", "history.txt", "-d", "F", "-a", "0.7"] + list(extra),
                              cwd=root, capture_output=True, text=True, timeout=300)
    for bad in ("15", "1025"):
        res = run("--sketch-size", bad)
        assert res.returncode == 2 and "--sketch-size" in res.stderr and ref.snapshot(root) == before
    res = run("-a", "80")
    assert res.returncode == 2 and "-a" in res.stderr and ref.snapshot(root) == before
    res = run("--report-floor", "1.5")
    assert res.returncode == 2 and "--report-floor" in res.stderr and ref.snapshot(root) == before
    tfa = os.path.join(root, "Clusters_fa", "Cluster_5_4.tfa")
    kept = open(tfa, "rb").read()
    os.remove(tfa)
    now = ref.snapshot(root)
    res = run()
    assert res.returncode == 1 and "Clusters_fa/Cluster_5_4.tfa" in res.stderr and ref.snapshot(root) == now
    open(tfa, "wb").close()
    now = ref.snapshot(root)
    res = run()
    assert res.returncode == 1 and "Clusters_fa/Cluster_5_4.tfa" in res.stderr and ref.snapshot(root) == now
    open(tfa, "wb").write(kept + b">toolong\n" + b"ACGT" * 8192 + b"\n")
    now = ref.snapshot(root)
    res = run()
    assert res.returncode == 1 and ">toolong" in res.stderr and "32768" in res.stderr and ref.snapshot(root) == now
    ctx = hip_lib.context(0)
    try:
        data, off = pack(["ACGT" * 8192, "ACGT" * 10])
        with pytest.raises(MprimeError, match="record 0 has 32768"):
            ctx.ani_sketch(data, off, 64)
        with pytest.raises(MprimeError, match="sketch size 8"):
            ctx.ani_sketch(data[:40], np.array([0, 40], np.int64), 8)
        with pytest.raises(MprimeError, match="mp_ani_sketch first"):
            ctx.ani_pairs([0], [0])
    finally:
        ctx.close()
