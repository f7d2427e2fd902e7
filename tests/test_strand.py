"""The both-strand yardstick (tests/strand_ref.py) on its own: the rc table, the invariants that tie it to the forward-only yardsticks,
the text the three command lines write with their flags, and the recorded run of the reference's own .clstr reader over a signed .clstr.
Nothing here needs a GPU."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import anchor_ref as aref
import cluster_cases
import cluster_ref as cref
import star_ref as sref
import strand_cases as cases
import strand_ref as ref
from conftest import GOLDEN, REPO


def test_rc_table():
    pairs = dict(A="T", T="A", C="G", G="C", R="Y", Y="R", K="M", M="K", B="V", V="B", D="H", H="D", S="S", W="W", N="N")
    for x, y in pairs.items():
        assert ref.rc(x) == y and ref.rc(x.lower()) == y
    assert ref.rc("U") == "A" and ref.rc("u") == "A"
    for foreign in "-.*?1 @[`{~\xe9":                   # no letter of the table: kept, and not upper-cased beyond a-z
        assert ref.rc(foreign) == foreign
    assert ref.rc("aCgTn-Ryk") == "MRY-NACGT" and ref.rc("") == "" and ref.rc(b"acg") == "CGT"
    iupac = "ACGTRYKMBVDHSWN"
    assert ref.rc(ref.rc(iupac + iupac.lower())) == iupac + iupac and ref.rc(ref.rc("GAUUACA")) == "GATTACA"
    # the code store: only A, C, G, T are complemented, every other letter keeps its (one) code
    assert ref.rc_codes("acgtURYn") == "NYRUACGT"
    # the library's table is the same one
    from multiprime_amd.anchor import oriented_id
    assert oriented_id(">x|1", True) == ">_R_x|1" == ref.oriented_id(">x|1", True) and oriented_id(">x", False) == ">x"


@pytest.fixture(scope="module")
def anchor_truth():
    groups = cases.anchor_groups()
    return groups, [cases.anchor_yardstick(g) for g in groups]


def test_orientation_of_the_planted_queries(anchor_truth):
    seen = 0
    for g, res in zip(*anchor_truth):
        a = g["anchor"]
        for q, planted, r in zip(g["queries"], g["planted"], res):
            cf, cr = ref.best_vote(q, a)[0], ref.best_vote(ref.rc(q), a)[0]
            assert r["reversed"] == (cr > cf) and bool(r["status"] & ref.REVERSED) == r["reversed"]
            assert r["reversed"] == planted or cf == cr, (g["name"], q)           # a draw stays as given, whatever was planted
            seen += r["reversed"]
    assert seen >= 40
    a = cases.anchor_300()
    own, drawn = cases.tie_queries(a)
    assert ref.rc(own) == own and ref.best_vote(own, a)[0] == 29
    assert ref.best_vote(drawn, a) == (9, 10) and ref.best_vote(ref.rc(drawn), a) == (9, 200) and not ref.orient(drawn, a)[1]
    assert ref.orient("ACGTACGTACG", a) == ("ACGTACGTACG", False)                 # under 12 bases: no vote either way


def test_a_mixed_set_equals_its_oriented_twin(anchor_truth):
    for g, res in zip(*anchor_truth):
        for q, r in zip(g["queries"], res):
            twin = ref.rc(q) if r["reversed"] else q
            want = aref.align(twin, g["anchor"], g["col"], g["width"], **g["params"])
            got = {k: v for k, v in r.items() if k != "reversed"}
            assert got == dict(want, status=want["status"] | (ref.REVERSED if r["reversed"] else 0))
            assert r["row"].replace("-", "") == _paired(ref.upper(twin), r["ops"]).replace("-", "")
            # fed pre-oriented, nothing is turned and the forward-only result comes back
            again = ref.align(twin, g["anchor"], g["col"], g["width"], **g["params"])
            assert not again["reversed"] and {k: v for k, v in again.items() if k != "reversed"} == want


def _paired(q, ops):
    """The query's bases that the ops pair with an anchor position (M), in order."""
    out, i = [], 0
    for op in ops:
        if op == "M":
            out.append(q[i])
        i += op != "D"
    assert i == len(q) or not ops
    return "".join(out)


def test_star_parity_and_twin():
    for g in cases.star_groups():
        res = cases.star_yardstick(g)
        assert res["parity"][-1] == g["planted"] and all(p == g["planted"] for p in res["parity"]), g["name"]       # turned once, in round 0
        twin = [ref.rc(r) if t else r for r, t in zip(g["records"], g["planted"])]
        fwd = sref.star(twin, rounds=g["rounds"], **g["params"])
        assert res["anchors"] == fwd["anchors"] and len(res["rounds"]) == len(fwd["rounds"])
        for a, b in zip(res["rounds"], fwd["rounds"]):
            assert a["rows"] == b["rows"] and a["ins"] == b["ins"] and a["width"] == b["width"] and a["counts"] == b["counts"]
            for q, (ma, mb) in enumerate(zip(a["meta"], b["meta"])):
                assert ma == dict(mb, status=mb["status"] | (ref.REVERSED if g["planted"][q] else 0))
        again = ref.star(twin, rounds=g["rounds"], **g["params"])
        assert not any(again["parity"][-1]) and [r["rows"] for r in again["rounds"]] == [r["rows"] for r in fwd["rounds"]]
        # a placed row without its gaps is the oriented record
        last = res["rounds"][-1]
        for rec, t, row in zip(g["records"], g["planted"], last["rows"]):
            assert row is None or row.replace("-", "") == (ref.rc(rec) if t else rec)
    names = [g["name"] for g in cases.star_groups()]
    drift = cases.star_yardstick(cases.star_groups()[names.index("drift-turned")])
    assert drift["rounds"][0]["meta"][1]["band"] == 64 and drift["rounds"][0]["meta"][1]["status"] & ref.REVERSED
    assert len(cases.star_yardstick(cases.star_groups()[names.index("consensus-turned")])["rounds"]) >= 2


@pytest.fixture(scope="module")
def family_truth():
    seqs, memo = cases.family_set(), {}
    return seqs, {p: ref.cluster(seqs, memo=memo, identity_permille=p) for p in (800, 900, 1000)}, memo


def test_clustering_both_strands(family_truth):
    seqs, truth, memo = family_truth             # (memo: the pair records, which do not depend on the identity asked for)
    assert len(seqs) == 48 and all(150 <= len(s) <= 400 for s in seqs)
    for permille, (cluster_of, reps, n_match_of, strand_of) in truth.items():
        fwd = cref.cluster(seqs, memo=memo, identity_permille=permille)
        assert len(reps) < len(fwd[1]) and sum(strand_of) > 0                     # forward only, the turned members split their families
        assert all(strand_of[r] == 0 and n_match_of[r] == len(seqs[r]) for r in reps)
        for i, k in enumerate(cluster_of):
            if i == reps[k]:
                continue
            plus = cref.similar(ref.upper(seqs[i]), seqs[reps[k]], memo=memo, identity_permille=permille)
            minus = cref.similar(ref.rc_codes(seqs[i]), seqs[reps[k]], memo=memo, identity_permille=permille)
            assert (strand_of[i], n_match_of[i]) == ((0, plus) if plus is not None else (1, minus))
            for r in reps[:k]:                                                    # no earlier representative on either strand
                assert ref.similar_pm(seqs[i], seqs[r], memo=memo, identity_permille=permille) is None
        # the twin, every member oriented to its representative: the forward-only rule gives the same clusters, and nothing is turned
        twin = [ref.rc_codes(s) if t else s for s, t in zip(seqs, strand_of)]
        assert tuple(cref.cluster(twin, memo=memo, identity_permille=permille)) == (cluster_of, reps, n_match_of)
        assert ref.cluster(twin, memo=memo, identity_permille=permille) == (cluster_of, reps, n_match_of, [0] * len(seqs))


def test_clustering_edges():
    seqs = cases.edge_set()
    at800, at1000 = ref.cluster(seqs, identity_permille=800), ref.cluster(seqs, identity_permille=1000)
    assert at800[0] == [0, 0, 0, 0, 1, 2, 0, 0, 0] and at800[3] == [0, 1, 1, 0, 0, 0, 1, 0, 1]
    assert at1000[0] == [0, 0, 1, 2, 3, 4, 0, 0, 0]          # the records with N found their own clusters; the 11-mers always do
    assert ref.pair(seqs[1], seqs[0], 1, identity_permille=1000)["n_match"] == 90 and ref.pair(seqs[1], seqs[0], 0)["status"] == 5


# ---- text -------------------------------------------------------------------------------------------------------------------------------
def test_clstr_lines_carry_the_strand(family_truth):
    from multiprime_amd.cluster import ClusterByIdentity
    seqs, truth, _ = family_truth
    ids = [i for i, _ in cluster_cases.named(seqs, "t")]
    cluster_of, reps, n_match_of, strand_of = truth[800]
    text = ref.clstr_text(ids, seqs, cluster_of, reps, n_match_of, strand_of)
    assert text.count("... at +/") + text.count("... at -/") + text.count("... *") == len(seqs) and text.count("... at -/") == sum(strand_of)
    app = ClusterByIdentity("in.fa", "out.fa", both_strands=True)
    app._ids, app.lens = ids, np.array([len(s) for s in seqs])
    app._cluster_of, app._reps, app._n_match, app._strand = (np.array(x, np.int32) for x in (cluster_of, reps, n_match_of, strand_of))
    assert app.clstr_text() == text and app.strand.tolist() == strand_of
    app.both_strands = False                             # without the flag the lines are the forward-only ones
    assert app.clstr_text() == cref.clstr_text(ids, seqs, cluster_of, reps, n_match_of)
    # the reference's reader takes the last blank-separated token as the identity string
    line = [x for x in text.splitlines() if "at -/" in x][0]
    assert line.split(" ")[-1].startswith("-/") and line.split(" ")[-1].endswith("%")


def _star_app(adjust, tmp_path, ids, records, res):
    from multiprime_amd.starmsa import StarAlignment
    last = res["rounds"][-1]
    app = StarAlignment("in.fa", str(tmp_path / ("star%d" % adjust)), adjust_direction=adjust)
    app._ids = ids
    app._rows = np.array([np.frombuffer((r or "-" * last["width"]).encode(), np.uint8) for r in last["rows"]])
    app._meta = np.array([[m["score"], m["d0"], m["n_match"], m["n_ins"], m["n_del"], m["first_col"], m["last_col"], m["status"], 0, 0, m["band"]]
                          for m in last["meta"]], np.int32)
    app.round_stats = [dict(n=len(a), width=r["width"], placed=sum(r["placed"]), band_warnings=sum(1 for m in r["meta"] if m["status"] & 2))
                       for a, r in zip(res["anchors"], res["rounds"])]
    raw = "".join(records).encode()
    app.raw, app.raw_off = np.frombuffer(raw, np.uint8), np.cumsum([0] + [len(r) for r in records])
    app.write()
    return [open(app.outfile + tail).read() for tail in ("", ".star.tsv", ".unaligned.fa")]


def test_star_files(tmp_path):
    g = cases.star_groups()[0]
    records = g["records"] + ["AG" * 30]                 # a stranger: unplaced, written as given
    ids = [">r%d" % q for q in range(len(records))]
    res = ref.star(records, rounds=1, **g["params"])
    fa, tsv, un = _star_app(True, tmp_path, ids, records, res)
    assert (fa, tsv, un) == ref.star_files(ids, records, res, True)
    assert fa.count(">_R_") == sum(g["planted"]) and ">_R_r1\n" in fa and un == ">r%d\n%s\n" % (len(records) - 1, "AG" * 30)
    lines = tsv.splitlines()
    assert lines[0].split("\t")[-1] == "strand" and [x.split("\t")[-1] for x in lines[1:5]] == ["+", "-", "+", "+"]
    fwd = sref.star(records, rounds=1, **g["params"])
    fa0, tsv0, un0 = _star_app(False, tmp_path, ids, records, fwd)
    assert (fa0, tsv0, un0) == ref.star_files(ids, records, fwd, False)
    assert tsv0.splitlines()[0].split("\t")[-1] == "n_del" and "_R_" not in fa0 and all(len(x.split("\t")) == 8 for x in tsv0.splitlines()[:-1])


def test_anchor_files(tmp_path):
    from multiprime_amd.anchor import AnchoredAlignment
    g = cases.anchor_groups()[3]                         # the letters group
    queries = g["queries"] + ["ag" * 30]
    ids = [">q%d" % q for q in range(len(queries))]
    n = len(g["anchor"])
    for adjust in (True, False):
        res = [(ref.align if adjust else aref.align)(q, g["anchor"], list(range(n)), n, **g["params"]) for q in queries]
        app = AnchoredAlignment("seed.fa", "in.fa", str(tmp_path / ("anchor%d" % adjust)), adjust_direction=adjust)
        app.seed_ids, app.seed_rows = [">seed"], np.frombuffer(g["anchor"].encode(), np.uint8).reshape(1, n)
        app._ids = ids
        app._rows = np.array([np.frombuffer(r["row"].encode(), np.uint8) for r in res])
        app._meta = np.array([[r["score"], r["d0"], r["n_match"], r["n_ins"], r["n_del"], r["first_col"], r["last_col"], r["status"], 0, 0] for r in res], np.int32)
        raw = "".join(queries).encode()
        app.qdata, app.qoff = np.frombuffer(raw, np.uint8), np.cumsum([0] + [len(q) for q in queries])
        app.write()
        got = [open(app.outfile + tail).read() for tail in ("", ".anchor.tsv", ".unaligned.fa")]
        assert got == list(ref.anchor_files([">seed"], [g["anchor"]], ids, queries, res, adjust))
        header = got[1].splitlines()[0].split("\t")
        assert (header[-1] == "strand" and ">_R_q0\n" in got[0] and ">_R_q2\n" in got[0]) if adjust else (header[-1] == "last_col" and "_R_" not in got[0])
        given = "".join("%s\n%s\n" % (i, q) for i, q in zip(ids, queries))
        # as given; forward only, the turned queries are rejected with the stranger
        assert got[2] == (">q3\n" + "ag" * 30 + "\n" if adjust else given.replace(">q1\n%s\n" % queries[1], ""))


@pytest.mark.parametrize("script, flags", [
    ("cluster_by_identity.py", ["-i", "x.fa", "-o", "y.fa", "--both-strands=yes"]),
    ("cluster_by_identity.py", ["-i", "x.fa", "-o", "y.fa", "--both-strands", "-c", "1.5"]),
    ("run_mafft.py", ["-i", "x.fa", "-o", "y.fa", "--adjust-direction=1"]),
    ("run_mafft.py", ["-i", "x.fa", "-o", "y.fa", "--adjust-direction", "--rounds", "0"]),
    ("anchor_msa.py", ["-s", "s.fa", "-i", "x.fa", "-o", "y.fa", "--adjust-direction", "both"]),
])
def test_flag_errors_exit_with_status_2(script, flags):
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts", script)] + flags, capture_output=True, text=True)
    assert r.returncode == 2 and "usage:" in r.stderr, (r.returncode, r.stderr)


def test_the_flags_reach_the_classes():
    from multiprime_amd import anchor, cluster, starmsa
    assert cluster.parse_args(["-i", "a", "-o", "b", "--both-strands"]).both_strands and not cluster.parse_args(["-i", "a", "-o", "b"]).both_strands
    assert starmsa.parse_args(["-i", "a", "-o", "b", "--adjust-direction"]).adjust_direction and not starmsa.parse_args(["-i", "a", "-o", "b"]).adjust_direction
    assert anchor.parse_args(["-s", "s", "-i", "a", "-o", "b", "--adjust-direction"]).adjust_direction
    assert not anchor.parse_args(["-s", "s", "-i", "a", "-o", "b"]).adjust_direction
    assert isinstance(cluster.ClusterByIdentity.strand, property)


# ---- the reference reads a signed .clstr ------------------------------------------------------------------------------------------------
def golden(name):
    with gzip.open(os.path.join(GOLDEN, name), "rt") as f:
        return f.read()


def test_the_reference_reads_a_signed_clstr():
    fa, clstr = golden("cluster_strands.fa.gz"), golden("cluster_strands.clstr.gz")
    ids, seqs = zip(*cref.read_fasta(fa))
    assert [(i, s) for i, s in zip(ids, seqs)] == [(i, s.upper()) for i, s in cases.mixed_set()]
    res = ref.cluster(list(seqs), identity_permille=800)
    assert ref.clstr_text(ids, seqs, *res) == clstr and 0 < sum(res[3]) < len(ids) - len(res[1])
    members = signed_members(clstr)
    txt = golden("cluster_strands.txt.gz").splitlines()
    assert txt[0] == "#Cluster_id\tNumber" and txt[1:] == ["Cluster_%d\t%d" % (k, len(m)) for k, m in enumerate(members)]
    want = ["Cluster_%d\t%s\t%s" % (k, ident[1:], tail) for k, m in enumerate(members) for ident, tail in m if tail != "*"]
    assert golden("cluster_strands.identities.txt.gz").splitlines() == want and len(want) == 27
    assert any(t.startswith("-/") for _, _, t in (x.split("\t") for x in want)) and any(t.startswith("+/") for _, _, t in (x.split("\t") for x in want))


def signed_members(clstr):
    """[[(id, '*' or '+/dd.dd%' or '-/dd.dd%')]] per cluster, written from the format lines alone."""
    out = []
    for line in clstr.splitlines():
        if line.startswith(">Cluster "):
            out.append([])
            continue
        rest = line.split("\t")[1].split("aa, ", 1)[1]
        ident, tail = rest.split("... ", 1)
        out[-1].append((ident, tail if tail == "*" else tail[len("at "):]))
    return out
