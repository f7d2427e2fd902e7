"""Both strands on the device — anchor_orient_kernel behind mp_anchor_strands in mp_anchor_align and mp_star_round, the reverse copies
of the code store behind mp_cluster_pairs_strands / mp_cluster_greedy_strands — against the yardstick of tests/strand_ref.py on the
cases of tests/strand_cases.py, field by field; with the switch off, the same calls against the forward-only yardsticks.  Then the
three scripts with their flags on one mixed set, and the recorded run of the reference's .clstr reader."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_cases
import cluster_ref as cref
import star_ref as sref
import strand_cases as cases
import strand_ref as ref
from anchor_ref import anchor_of
from conftest import GOLDEN, REPO
from multiprime_amd._abi import ANCHOR_REVERSED, MprimeError
from multiprime_amd.starmsa import anchor_of_counts

FIELDS = ("score", "d0", "n_match", "n_ins", "n_del", "first_col", "last_col", "status")
PAIR_FIELDS = ("votes", "d0", "score", "n_match", "status")
IDENTITIES = (800, 900, 1000)


def pack(records):
    raw = [q.encode() for q in records]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw), np.uint8), off


# ---- anchored alignment -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def anchor_truth():
    """Per group the yardstick with both strands and the forward-only yardstick, computed once."""
    groups = cases.anchor_groups()
    return groups, [cases.anchor_yardstick(g) for g in groups], [cases.anchor_yardstick(g, strands=False) for g in groups]


def device(ctx, g, queries=None, want_ops=True):
    ctx.anchor_set(g["anchor"].encode(), g["col"], g["width"], **g["params"])
    data, off = pack(g["queries"] if queries is None else queries)
    given = data.copy()
    rows, meta, ops = ctx.anchor_align(data, off, want_ops=want_ops)
    assert (data == given).all()                          # the caller's bytes are never turned
    ops = [op.decode() for op in ops] if want_ops else [None] * len(rows)
    return [dict(zip(FIELDS, mt[:8]), row=row.tobytes().decode(), ops=op) for row, mt, op in zip(rows, meta.tolist(), ops)]


def same(got, want, what):
    assert len(got) == len(want), what
    for q, (a, b) in enumerate(zip(got, want)):
        for key in FIELDS + ("ops", "row"):
            assert a[key] == b[key], (what, q, key, a[key], b[key])


@pytest.mark.gpu
def test_anchor_groups_equal_the_yardstick(hip_lib, anchor_truth):
    assert hip_lib.backend == "hip" and hip_lib.strands
    ctx = hip_lib.context(0)
    try:
        ctx.anchor_strands(True)
        turned = 0
        for g, want, _ in zip(*anchor_truth):
            got = device(ctx, g)
            same(got, want, g["name"])
            turned += sum(1 for r in got if r["status"] & ANCHOR_REVERSED)
            if g["name"] == "draws":
                assert [r["status"] & ANCHOR_REVERSED for r in got] == [0, 0]
            if g["name"] == "lengths":                    # odd and even m up to two passes of the in-place swap
                assert [bool(r["status"] & ANCHOR_REVERSED) for r in got] == g["planted"]
        assert turned >= 40
        # the switch off again: the forward-only rule on the same calls, bit 3 never set
        ctx.anchor_strands(False)
        for g, _, fwd in zip(*anchor_truth):
            got = device(ctx, g)
            same(got, fwd, g["name"] + " (forward)")
            assert not any(r["status"] & ANCHOR_REVERSED for r in got)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_anchor_without_the_switch_is_forward_only(hip_lib, anchor_truth):
    """A context that never heard of the switch."""
    ctx = hip_lib.context(0)
    try:
        for g, _, fwd in zip(*anchor_truth):
            same(device(ctx, g), fwd, g["name"])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_anchor_turns_do_not_leak_across_batches(hip_lib, anchor_truth, monkeypatch):
    g, want, _ = next(x for x in zip(*anchor_truth) if x[0]["name"] == "family-half-turned")
    monkeypatch.setenv("MP_ANCHOR_BATCH", "3")
    ctx = hip_lib.context(0)
    try:
        ctx.anchor_strands(True)
        same(device(ctx, g), want, "batch 3")
        assert ctx.anchor_stats()[1]["batches"] == (len(want) + 2) // 3
        # without ops: the same rows and records
        got = device(ctx, g, want_ops=False)
        assert [r["row"] for r in got] == [w["row"] for w in want] and [[r[k] for k in FIELDS] for r in got] == [[w[k] for k in FIELDS] for w in want]
        # ops of a turned query alone
        q = g["planted"].index(True)
        same(device(ctx, g, [g["queries"][q]]), [want[q]], "one turned query")
        assert want[q]["status"] & ANCHOR_REVERSED and want[q]["ops"]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_a_turned_query_at_the_length_limit(hip_lib):
    g = cases.long_group()
    want = cases.anchor_yardstick(g)
    assert len(g["queries"][0]) == 32767 and want[0]["status"] == 3 | ANCHOR_REVERSED and want[0]["d0"] == -19980
    ctx = hip_lib.context(0)
    try:
        ctx.anchor_strands(True)
        same(device(ctx, g), want, "limit")
        ctx.anchor_strands(False)
        got = device(ctx, g)
        assert got[0]["status"] == 3 and got[0]["d0"] != want[0]["d0"]
    finally:
        ctx.close()


# ---- star alignment ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def star_truth():
    groups = cases.star_groups()
    return groups, [cases.star_yardstick(g) for g in groups]


def device_round(ctx, anchor, params):
    """One round as the yardstick's dict, plus the anchor its counts lead to."""
    meta, ins, width = ctx.star_round(anchor.encode(), **params)
    rows, counts = ctx.star_rows(), ctx.star_counts()
    placed = (meta[:, 7] & 1) == 0
    return dict(rows=[r.tobytes().decode() if ok else None for r, ok in zip(rows, placed)],
                meta=[dict(zip(FIELDS + ("band",), mt[:8] + [mt[10]])) for mt in meta.tolist()], ins=ins.tolist(), width=width,
                counts=counts.tolist(), placed=placed.tolist(), next_anchor=anchor_of_counts(counts, int(placed.sum())).decode())


def same_round(got, want, what):
    for key in ("width", "ins", "placed", "counts"):
        assert got[key] == want[key], (what, key)
    for q, (a, b) in enumerate(zip(got["meta"], want["meta"])):
        assert a == b, (what, q, a, b)
    assert got["rows"] == want["rows"], what
    assert got["next_anchor"] == anchor_of([r for r in want["rows"] if r is not None])[0], what


def same_group(ctx, g, want):
    ctx.star_load(*pack(g["records"]))
    for k, (anchor, rnd) in enumerate(zip(want["anchors"], want["rounds"])):
        same_round(device_round(ctx, anchor, g["params"]), rnd, (g["name"], k))


@pytest.mark.gpu
@pytest.mark.parametrize("batch", (None, 5))
def test_star_groups_equal_the_yardstick(batch, hip_lib, star_truth, monkeypatch):
    if batch is None:
        monkeypatch.delenv("MP_STAR_BATCH", raising=False)
    else:
        monkeypatch.setenv("MP_STAR_BATCH", str(batch))
    ctx = hip_lib.context(0)
    try:
        ctx.anchor_strands(True)
        for g, want in zip(*star_truth):
            same_group(ctx, g, want)
            if batch is not None:
                assert ctx.star_stats()[1]["batches"] == (len(g["records"]) + batch - 1) // batch
        names = [g["name"] for g in star_truth[0]]
        drift = star_truth[1][names.index("drift-turned")]["rounds"][0]["meta"][1]
        assert drift["band"] == 64 and drift["status"] & ANCHOR_REVERSED          # a turned record that escalated its band
        assert len(star_truth[1][names.index("consensus-turned")]["rounds"]) >= 2   # two rounds: the parity did not flip twice
    finally:
        ctx.close()


@pytest.mark.gpu
def test_star_load_clears_the_parity(hip_lib, star_truth):
    g, want = star_truth[0][0], star_truth[1][0]
    ctx = hip_lib.context(0)
    try:
        ctx.anchor_strands(True)
        same_group(ctx, g, want)
        # the same round once more on the records as they are held now: nothing is turned again, the parity stays
        same_round(device_round(ctx, want["anchors"][-1], g["params"]), want["rounds"][-1], "held")
        same_group(ctx, g, want)                          # loaded again: as given, parity 0, turned afresh
        # the switch off on freshly loaded records: the forward-only yardstick
        ctx.anchor_strands(False)
        ctx.star_load(*pack(g["records"]))
        fwd = sref.star_round(g["records"], want["anchors"][0], **g["params"])
        got = device_round(ctx, want["anchors"][0], g["params"])
        same_round(got, fwd, "forward")
        assert not any(m["status"] & ANCHOR_REVERSED for m in got["meta"]) and got["rows"] != want["rounds"][0]["rows"]
    finally:
        ctx.close()


# ---- clustering -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair_truth():
    """All ordered pairs x both strands of the 20 records, the yardstick's record per band."""
    seqs = cases.pair_set()
    n = len(seqs)
    q, r, s = np.unravel_index(np.arange(n * n * 2), (n, n, 2))
    want = {W: [ref.pair(seqs[a], seqs[b], int(st), band=W, identity_permille=800) for a, b, st in zip(q, r, s)] for W in (0, 32, 255)}
    return seqs, q.astype(np.int32), r.astype(np.int32), s.astype(np.int32), want


@pytest.mark.gpu
@pytest.mark.parametrize("W", (0, 32, 255))
def test_pairs_on_both_strands(W, hip_lib, pair_truth):
    seqs, q, r, s, want = pair_truth
    assert len(seqs) == 20
    ctx = hip_lib.context(0)
    try:
        ctx.cluster_load(*pack(seqs))
        got = ctx.cluster_pairs_strands(q, r, s, band=W, identity_permille=800).tolist()
        aligned = [0, 0]
        for x, (g, w) in enumerate(zip(got, want[W])):
            assert dict(zip(PAIR_FIELDS, g)) == w, (W, int(q[x]), int(r[x]), int(s[x]), g, w)
            aligned[int(s[x])] += w["status"] != 5
        assert min(aligned) > 20 and ctx.cluster_stats()[1]["pairs"] == sum(aligned)
        # strand 0 of that call is mp_cluster_pairs, also after the store has grown
        fwd = ctx.cluster_pairs(q[s == 0], r[s == 0], band=W, identity_permille=800).tolist()
        assert fwd == [g for g, st in zip(got, s) if st == 0]
        with pytest.raises(MprimeError, match="strand 2"):
            ctx.cluster_pairs_strands([0], [1], [2])
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def greedy_truth():
    seqs, memo = cases.family_set(), {}
    return seqs, {p: ref.cluster(seqs, memo=memo, identity_permille=p) for p in IDENTITIES}, {p: cref.cluster(seqs, memo=memo, identity_permille=p) for p in IDENTITIES}


def greedy_strands(hip_lib, seqs, **kw):
    ctx = hip_lib.context(0)
    try:
        ctx.cluster_load(*pack(seqs))
        return tuple(x.tolist() for x in ctx.cluster_greedy_strands(**kw)), ctx.cluster_stats()[1]
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("block", (None, 1, 2, 7))
def test_greedy_on_both_strands_for_every_block(block, hip_lib, greedy_truth, monkeypatch):
    if block is None:
        monkeypatch.delenv("MP_CLUSTER_BLOCK", raising=False)
    else:
        monkeypatch.setenv("MP_CLUSTER_BLOCK", str(block))
    seqs, both, _ = greedy_truth
    for permille in IDENTITIES:
        got, counts = greedy_strands(hip_lib, seqs, identity_permille=permille)
        assert got == tuple(both[permille]), (block, permille)
        if block is not None:
            assert counts["rounds"] >= (len(both[permille][1]) + block - 1) // block


@pytest.mark.gpu
def test_greedy_on_both_strands_with_a_small_pair_batch(hip_lib, greedy_truth, monkeypatch):
    monkeypatch.setenv("MP_CLUSTER_PAIR_BATCH", "7")
    monkeypatch.setenv("MP_CLUSTER_BLOCK", "5")
    seqs, both, _ = greedy_truth
    assert greedy_strands(hip_lib, seqs, identity_permille=800)[0] == tuple(both[800])
    # min_votes = 0: every pair is aligned on the forward strand, and on the reverse strand where that did not hold
    small = seqs[:12]
    got, counts = greedy_strands(hip_lib, small, identity_permille=800, min_votes=0)
    assert got == tuple(ref.cluster(small, identity_permille=800, min_votes=0))


@pytest.mark.gpu
def test_the_forward_call_still_splits_the_families(hip_lib, greedy_truth):
    seqs, both, fwd = greedy_truth
    ctx = hip_lib.context(0)
    try:
        ctx.cluster_load(*pack(seqs))
        for permille in IDENTITIES:
            got = tuple(x.tolist() for x in ctx.cluster_greedy(identity_permille=permille))
            assert got == tuple(fwd[permille]) and len(got[1]) > len(both[permille][1])
        # and after a both-strand call has doubled the store
        assert tuple(x.tolist() for x in ctx.cluster_greedy_strands(identity_permille=800)) == tuple(both[800])
        assert tuple(x.tolist() for x in ctx.cluster_greedy(identity_permille=800)) == tuple(fwd[800])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_short_records_and_n_on_both_strands(hip_lib):
    seqs = cases.edge_set()
    for permille in (800, 1000):
        assert greedy_strands(hip_lib, seqs, identity_permille=permille)[0] == tuple(ref.cluster(seqs, identity_permille=permille))


# ---- the scripts end to end -------------------------------------------------------------------------------------------------------------
def golden(name):
    with gzip.open(os.path.join(GOLDEN, name), "rt") as f:
        return f.read()


def run(script, *flags):
    return subprocess.run([sys.executable, os.path.join(REPO, "scripts", script), *flags], capture_output=True, text=True)


@pytest.mark.gpu
def test_the_three_scripts_on_a_mixed_set(hip_lib, tmp_path):
    records = cases.mixed_set()
    ids, seqs = [i for i, _ in records], [s for _, s in records]
    inp = tmp_path / "in.fa"
    inp.write_text(cluster_cases.fasta(records))
    # clustering on both strands
    r = run("cluster_by_identity.py", "-i", str(inp), "-o", str(tmp_path / "c80.fa"), "-c", "0.8", "--both-strands")
    assert r.returncode == 0 and "Total times" in r.stdout, r.stderr
    want = ref.cluster(seqs, identity_permille=800)
    clstr = (tmp_path / "c80.fa.clstr").read_text()
    assert clstr == ref.clstr_text(ids, seqs, *want) and (tmp_path / "c80.fa").read_text() == cref.rep_fasta(ids, seqs, want[1])
    # ... reproduces what the reference's reader saw in the yardstick's file (tests/golden/make_golden_cluster_strands.py)
    assert clstr == golden("cluster_strands.clstr.gz")
    members = []
    for line in clstr.splitlines():
        if line.startswith(">Cluster "):
            members.append([])
        else:
            members[-1].append(line)
    # (as the reference reads a member line: the id between '>' and '...', the identity string the last blank-separated token)
    seen = ["Cluster_%d\t%s\t%s" % (k, line.split(">")[1].split("...")[0], line.split(" ")[-1]) for k, m in enumerate(members) for line in m
            if line.split(" ")[-1] != "*"]
    assert seen == golden("cluster_strands.identities.txt.gz").splitlines()
    assert ["Cluster_%d\t%d" % (k, len(m)) for k, m in enumerate(members)] == golden("cluster_strands.txt.gz").splitlines()[1:]
    # forward only, the same set falls apart
    r = run("cluster_by_identity.py", "-i", str(inp), "-o", str(tmp_path / "fwd.fa"), "-c", "0.8")
    assert r.returncode == 0 and (tmp_path / "fwd.fa.clstr").read_text() == cref.clstr_text(ids, seqs, *cref.cluster(seqs, identity_permille=800))
    assert (tmp_path / "fwd.fa.clstr").read_text().count(">Cluster") > len(want[1])
    # the largest cluster's members as they stand in the input: the star alignment orients them
    k = max(range(len(want[1])), key=lambda k: want[0].count(k))
    mem = [i for i in range(len(ids)) if want[0][i] == k]
    mids, mseqs = [ids[i] for i in mem], [seqs[i] for i in mem]
    tfa = tmp_path / "cluster.tfa"
    tfa.write_text("".join("%s\n%s\n" % x for x in zip(mids, mseqs)))
    r = run("run_mafft.py", "-i", str(tfa), "-o", str(tmp_path / "cluster.tmsa"), "--adjust-direction")
    assert r.returncode == 0, r.stderr
    res = ref.star(mseqs, rounds=2)
    fa, tsv, un = ref.star_files(mids, mseqs, res, True)
    assert [(tmp_path / ("cluster.tmsa" + t)).read_text() for t in ("", ".star.tsv", ".unaligned.fa")] == [fa, tsv, un]
    assert fa.count(">_R_") == sum(res["parity"][-1]) > 0 and un == ""
    r = run("run_mafft.py", "-i", str(tfa), "-o", str(tmp_path / "fwd.tmsa"))
    fwd = sref.star(mseqs, rounds=2)
    assert r.returncode == 0 and [(tmp_path / ("fwd.tmsa" + t)).read_text() for t in ("", ".star.tsv", ".unaligned.fa")] == list(ref.star_files(mids, mseqs, fwd, False))
    # anchored alignment of every record of the set onto that alignment
    seed_ids, seed_rows = zip(*cref.read_fasta(fa))
    r = run("anchor_msa.py", "-s", str(tmp_path / "cluster.tmsa"), "-i", str(inp), "-o", str(tmp_path / "full.tmsa"), "--adjust-direction")
    assert r.returncode == 0, r.stderr
    anchor, col = anchor_of(seed_rows)
    results = [ref.align(s, anchor, col, len(seed_rows[0]), min_identity_permille=500) for s in seqs]
    want_files = ref.anchor_files(seed_ids, seed_rows, ids, seqs, results, True)
    assert [(tmp_path / ("full.tmsa" + t)).read_text() for t in ("", ".anchor.tsv", ".unaligned.fa")] == list(want_files)
    assert sum(1 for x in results if x["status"] & ANCHOR_REVERSED and not x["status"] & 1) >= 5 and want_files[1].splitlines()[0].endswith("\tstrand")
