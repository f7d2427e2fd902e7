"""The identity merge without a GPU: the yardstick of tests/ani_ref.py on the cases of tests/ani_cases.py (each named situation really
occurs), the library's table against math.log, and the host side of multiprime_amd/animerge.py — decide / apply driven by the
yardstick's numbers — against the reference scripts' recorded behaviour (tests/golden/ani_small.json.gz) and against the yardstick's
own decision and file operations for -a, -t, equal sizes and a chain."""
import os

import pytest

import ani_cases as cases
import ani_ref as ref
from conftest import load_gz_json
from multiprime_amd.animerge import merge_clstr


# ---- the yardstick on the cases ------------------------------------------------------------------------------------------------------------
def test_sketch_cases_are_what_their_labels_say():
    recs = dict(cases.sketch_records())
    for n in (8, 11):
        assert ref.sketch(recs["len %d" % n]) == []
    assert len(ref.sketch(recs["len 12"])) == 1 and len(ref.words(recs["len 13"])) == 2 and len(ref.words(recs["len 1035"])) == 1024
    for s in cases.SKETCH_SIZES:
        for d in (-1, 0, 1):
            seq = recs["words %d%+d" % (s, d)]
            assert len(ref.words(seq)) == s + d                # distinct
            assert len(ref.sketch(seq, s)) == min(s, s + d)    # one short of full, full, full with one hash left out
        assert ref.sketch(recs["words %d+1" % s], s) == sorted(ref.fmix32(v) for v in ref.words(recs["words %d+1" % s]))[:-1]
    assert len(ref.words(recs["500 x A"])) == 1 and ref.sketch(recs["500 x A"]) == [ref.fmix32(0)]
    assert len(ref.words(recs["tandem repeat"])) == 10
    assert ref.words(recs["N every 10 bases"]) == set() and ref.sketch(recs["empty"]) == []
    assert len(ref.words(recs["one N in the middle"])) == 300 - 11 - 12
    assert ref.sketch(recs["lower case"]) == ref.sketch(recs["lower case"].upper()) and len(ref.sketch(recs["lower case"])) == 689
    for n in cases.SORT_SIZES:
        assert [len(recs["sort size %d%+d" % (n, d)]) - 11 for d in (-1, 0, 1)] == [n - 1, n, n + 1]
    assert len(recs["32767 bases"]) == 32767
    sk = ref.sketch(recs["32767 bases"], 100)
    assert sk == sorted(set(sk)) and len(sk) == 100


def test_hash_and_table():
    assert ref.fmix32(0) == 0 and ref.fmix32(1) == 0x514E28B7 and ref.fmix32(0x331DA083) == 0xFFFFFFFF
    assert len({ref.fmix32(v) for v in range(1 << 16)}) == 1 << 16
    assert ref.words("ACGTACGTACGT") == {0x1B1B1B} and ref.words("acgtacgtacgN") == set()
    tab = ref.TAB
    assert len(tab) == 1025 and tab[0] == 0 and tab[1024] == 1000000 and all(a <= b for a, b in zip(tab, tab[1:]))
    assert tab[1] == 480058 and tab[512] == 966211             # 1 + ln(2 / 1025) / 12 = 0.4800582, 1 + ln(2 / 3) / 12 = 0.9662112


def test_pair_cases_cover_the_rule():
    seqs = cases.pair_records()
    assert 55 <= len(seqs) <= 65
    seen = set()
    for s in (16, 100, 1024):
        sk = [ref.sketch(x, s) for x in seqs]
        full = [len(x) == s for x in sk]
        assert any(full) and any(not f and x for f, x in zip(full, sk)) and sum(1 for x in sk if not x) >= 4
        for a in range(len(sk)):
            for b in range(a, len(sk)):
                w, u, ani = ref.pair(sk[a], sk[b], s)
                assert ref.pair(sk[b], sk[a], s) == (w, u, ani) and 0 <= w <= u <= 2 * s
                seen.add((full[a], full[b], ani >= 700000, u == 0))
    assert {(True, True, True, False), (True, False, True, False), (False, False, True, False), (False, False, False, True),
            (True, True, False, False)} <= seen
    a, b = ref.sketch(seqs[33], 1024), ref.sketch(seqs[34], 1024)   # the root of 1500 bases and its copy
    assert ref.pair(a, b, 1024) == (1024, 1024, 1000000)
    # a full sketch against a non-full one: only hashes up to the full one's last count on either side
    big, small = ref.sketch(seqs[45], 100), ref.sketch(seqs[1], 100)
    assert len(big) == 100 and 0 < len(small) < 100
    w, u, _ = ref.pair(big, small, 100)
    assert u == 100 + sum(1 for x in small if x <= big[-1]) - w


def test_group_cases_cover_the_rule():
    records, groups = cases.group_records()
    assert [len(g) for g in groups[:5]] == [1, 63, 64, 65, 500]
    for s in (64, 1024):
        sk = [ref.sketch(x, s) for x in records]
        of = lambda g: [sk[i] for i in g]
        assert all(not sk[i] for i in groups[5]) and ref.groups(of(groups[5]), of(groups[5]), s, 0) == (25, 0)
        assert ref.groups(of(groups[5]), of(groups[1]), s, 1) == (0, 0)
        assert ref.groups(of(groups[0]), of(groups[6]), s, 700000) == (0, 0)         # unrelated families: nothing reported
        n_rep, total = ref.groups(of(groups[0]), of(groups[1]), s, 700000)
        assert 0 < n_rep < 63 and 700000 * n_rep <= total < 1000000 * n_rep
        assert ref.groups(of(groups[0]), of(groups[1]), s, 0)[0] == 63
        n_one = ref.groups(of(groups[6]), of(groups[6]), s, 1000000)
        assert n_one[0] >= 8 and n_one[1] == 1000000 * n_one[0]                      # a record against itself and against its copy


def test_table_of_the_library_equals_the_yardstick():
    import __graft_entry__ as g
    g.build()
    from multiprime_amd._abi import Library
    assert Library(g.HIP_SO).ani_table().tolist() == ref.TAB


def test_records_from_memory():
    """merge_clstr(clusters=...) + load_records(): the device pass's input without files (tools/ani_bench.py); the list is sorted as
    cluster.txt's is and the offsets must split the records into its clusters."""
    import numpy as np
    app = merge_clstr(clusters=[("a", 2), ("b", 5), ("c", 2)], threshold=0, ani=0.8)
    assert app.cluster == [("b", 5), ("a", 2), ("c", 2)] and app.visiting() == [2, 1, 0] and app.work_dir == "Clusters_fa"
    data, off = np.frombuffer(b"ACGT" * 9, np.uint8), np.arange(10, dtype=np.int64) * 4
    app.load_records(data, off, [0, 5, 7, 9])
    assert app._group_off.tolist() == [0, 5, 7, 9] and app._off is off
    for bad in ([0, 5, 7], [0, 5, 7, 8], [1, 5, 7, 9], [0, 7, 5, 9]):
        with pytest.raises(ValueError, match="group_off"):
            app.load_records(data, off, bad)
    with pytest.raises(ValueError, match="record 1 has 40000"):
        app.load_records(np.zeros(40008, np.uint8), np.array([0, 4, 40004, 40008] + [40008] * 6, np.int64), [0, 5, 7, 9])
    assert app.decide({(2, 0): (0, 0), (1, 0): (3, 2400000)}) == {"Clusters_fa/b_5": ["Clusters_fa/a_2"]}


# ---- the reference pin ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return load_gz_json("ani_small.json.gz")


def as_bytes(tree):
    return {k: (None if v is None else v.encode()) for k, v in tree.items()}


@pytest.mark.parametrize("mode", ["T", "F"])
def test_decide_and_apply_equal_the_reference(mode, golden, tmp_path, monkeypatch):
    """The unmodified reference scripts ran on this tree with a stand-in fastANI that printed the yardstick's reported pairs
    (tests/golden/make_golden_ani.py).  With -a at the floor our decision is the reference's: history.txt and every file, byte for byte."""
    meta = golden["meta"]
    ref.restore(str(tmp_path), as_bytes(golden["input"]))
    monkeypatch.chdir(tmp_path)
    app = merge_clstr(inputfile="cluster.txt", output="history.txt", threshold=meta["t"], drop=mode, ani=meta["a"], nproc=1,
                      sketch_size=meta["s"], report_floor=meta["floor"])
    assert app.work_dir == "Clusters_fa" and app.cluster == ref.parse_clusters(golden["input"]["cluster.txt"])
    app.decide(ref.tree_numbers(app.cluster, app.work_dir, meta["s"], int(meta["floor"] * 1e6)))
    app.write_history()
    app.apply()
    got, want = ref.snapshot(str(tmp_path)), as_bytes(golden[mode])
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k
    lines = [x.split("\t") for x in golden[mode]["history.txt"].splitlines()]
    assert len(lines) == 5 and not {r for r, _ in lines} & {s for _, s in lines}        # merges, and no chain among them
    assert golden["T"]["history.txt"] == golden["F"]["history.txt"]
    assert ("Clusters_fa/Cluster_0_11.tfa" in want) == (mode == "F") and "Clusters_fa/Cluster_1_3.fa" not in want


# ---- -a, -t, equal sizes, a chain: against the yardstick -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def semantics(tmp_path_factory):
    """The tree of ani_cases.semantics_clusters, its snapshot and the yardstick's numbers for every cluster pair (computed once)."""
    root = tmp_path_factory.mktemp("ani_sem")
    cases.write_tree(str(root), cases.semantics_clusters())
    clusters = ref.parse_clusters(open(os.path.join(str(root), "cluster.txt")).read())
    numbers = ref.tree_numbers(clusters, os.path.join(str(root), "Clusters_fa"), 1024, 700000)
    table = {(p, r): numbers(p, r) for p in range(len(clusters)) for r in range(len(clusters))}
    return ref.snapshot(str(root)), clusters, table


def run_both(tmp_path, semantics, t, a, drop):
    """decide / apply of the product and of the yardstick on fresh copies of the tree: (history text, {sub name: ref name})."""
    snap, clusters, table = semantics
    out = []
    for who in ("product", "yardstick"):
        root = str(tmp_path / who)
        ref.restore(root, snap)
        cf, wd = os.path.join(root, "cluster.txt"), os.path.join(root, "Clusters_fa")
        if who == "product":
            app = merge_clstr(inputfile=cf, output=os.path.join(root, "history.txt"), threshold=t, drop=drop, ani=a)
            assert app.cluster == clusters and app.work_dir == wd == ref.work_dir(cf)
            app.decide(table)
            app.write_history()
            app.apply()
        else:
            md = ref.merge_dict(clusters, wd, ref.decide(clusters, t, int(round(a * 1e6)), lambda p, r: table[(p, r)]))
            open(os.path.join(root, "history.txt"), "w").write(ref.history_text(md))
            ref.apply(clusters, wd, md, drop)
        out.append({k: (v if v is None else v.replace(root.encode(), b"ROOT")) for k, v in ref.snapshot(root).items()})
    assert out[0] == out[1]
    hist = out[0]["history.txt"].decode()
    name = lambda x: os.path.basename(x).rsplit("_", 1)[0]
    return out[0], {name(s): name(r) for r, s in (x.split("\t") for x in hist.splitlines())}


def test_cases_land_where_intended(semantics):
    _, clusters, table = semantics
    pos = {name: x for x, (name, _) in enumerate(clusters)}
    assert [name for name, _ in clusters] == ["R", "L", "Q", "E1", "M", "E2", "P", "U"]
    mean = lambda p, r: table[(pos[p], pos[r])][1] / max(1, table[(pos[p], pos[r])][0])
    full = lambda p, r: table[(pos[p], pos[r])][0] == clusters[pos[p]][1] * clusters[pos[r]][1]
    assert full("P", "Q") and full("Q", "R") and mean("P", "Q") >= 850000 and mean("Q", "R") >= 850000       # 11 % per hop
    assert full("P", "R") and 700000 <= mean("P", "R") < 800000                                             # two hops: reported, below 0.8
    assert full("M", "L") and 700000 <= mean("M", "L") < 800000                                             # 22 %
    assert full("E2", "E1") and mean("E2", "E1") >= 900000                                                  # equal sizes, close
    for other in ("R", "L", "Q", "E1", "M", "E2", "P"):
        assert table[(pos["U"], pos[other])] == (0, 0)                                                       # unrelated: nothing reported
    assert table[(pos["M"], pos["R"])] == (0, 0) and table[(pos["E1"], pos["R"])] == (0, 0)


def test_a_is_a_fraction_of_the_mean(tmp_path, semantics):
    _, at8 = run_both(tmp_path / "a8", semantics, 20, 0.8, "T")
    _, at7 = run_both(tmp_path / "a7", semantics, 20, 0.7, "T")
    assert at8 == {"P": "Q", "Q": "R"}                         # M's pairs are reported but average below 0.8; P passes R by for Q
    assert at7 == {"P": "R", "Q": "R", "M": "L"}               # at the floor every reported pair merges, as in the reference


def test_threshold_0_visits_all_and_1_visits_none(tmp_path, semantics):
    tree1, none = run_both(tmp_path / "t1", semantics, 1, 0.7, "T")
    assert none == {} and tree1["history.txt"] == b"" and "Clusters_fa/P_2.fa" in tree1 and "Clusters_fa/P_2" not in tree1
    _, every = run_both(tmp_path / "t0", semantics, 0, 0.7, "T")
    assert every == {"P": "R", "Q": "R", "M": "L"}
    _, small = run_both(tmp_path / "t2", semantics, 2, 0.7, "T")
    assert small == {"P": "R"}                                 # Q (4) and M (3) are not rare at -t 2


def test_equal_sizes_are_never_compared(tmp_path, semantics):
    snap, clusters, table = semantics
    looked = []
    ref.restore(str(tmp_path), snap)
    app = merge_clstr(inputfile=str(tmp_path / "cluster.txt"), output=str(tmp_path / "h.txt"), threshold=0, ani=0.7)
    app.decide(lambda p, r: looked.append((p, r)) or table[(p, r)])
    assert looked and all(clusters[r][1] > clusters[p][1] for p, r in looked)
    assert not any("E1" in k or "E2" in k for k in app.merge_dict) and not any("E" in s for v in app.merge_dict.values() for s in v)


@pytest.mark.parametrize("drop", ["T", "F"])
def test_a_chain_in_both_modes(drop, tmp_path, semantics):
    tree, merged = run_both(tmp_path, semantics, 20, 0.8, drop)
    assert merged == {"P": "Q", "Q": "R"}
    assert tree["history.txt"].decode().splitlines() == ["ROOT/Clusters_fa/Q_4\tROOT/Clusters_fa/P_2", "ROOT/Clusters_fa/R_8\tROOT/Clusters_fa/Q_4"]
    files = sorted(k for k in tree if k.startswith("Clusters_fa/") and k.endswith(".tfa"))
    snap = semantics[0]
    if drop == "T":                                            # P goes; Q is itself a ref and stays, as in the reference
        assert files == ["Clusters_fa/%s.tfa" % x for x in ("E1_3", "E2_3", "L_6", "M_3", "Q_4", "R_8", "U_1")]
    else:                                                      # Q receives P first, then R receives what Q has become
        assert files == ["Clusters_fa/%s.tfa" % x for x in ("E1_3", "E2_3", "L_6", "M_3", "R_14", "U_1")]
        for ext in (".fa", ".tfa", ".txt"):
            assert tree["Clusters_fa/R_14" + ext] == snap["Clusters_fa/R_8" + ext] + snap["Clusters_fa/Q_4" + ext] + snap["Clusters_fa/P_2" + ext]
    assert not any(v is None and k != "Clusters_fa" for k, v in tree.items())           # the per-sequence directories are gone
