"""The both-strand rule of include/mprime_ani.h on the host alone: the yardstick tests/ani_strand_ref.py against the forward yardstick
tests/ani_ref.py on the cases of tests/ani_cases.py, then what merge_cluster_by_ANI.py does with a strand per merge (the .strand file,
--orient in apply(), the refused flag combinations) with the strands injected — no device."""
import os
import random
import subprocess
import sys

import pytest

import ani_cases as cases
import ani_ref as ref
import ani_strand_ref as sref
from anchor_cases import rand_seq
from conftest import REPO
from multiprime_amd.animerge import merge_clstr

SCRIPT = os.path.join(REPO, "scripts", "merge_cluster_by_ANI.py")
ALL = 1 << 30                                   # a sketch size no record fills


def test_word_rc_and_rc():
    assert sref.rc("ACGTNacgtnRYKMSWHBVD-x") == "x-HBVDWSKMRYnacgtNACGT"
    for seq in ("ACGTACGTTTGA", "AAAAAAAAAAAA", "ACGTACGTACGT", "GATTACAGATTA"):
        (f,), (r,) = ref.words(seq), ref.words(sref.rc(seq))
        assert sref.word_rc(f) == r and sref.word_rc(r) == f
    (pal,) = ref.words("ACGTACGTACGT")
    assert sref.word_rc(pal) == pal


@pytest.fixture(scope="module")
def records():
    return [seq for _, seq in cases.sketch_records()] + cases.pair_records()


def test_canonical_sketch_against_the_forward_words(records):
    """Hashes: the forward words' min(f, rc f), hashed.  Bits: 0 iff the canonical word itself is a forward word of the record.  The
    reverse complement has the same hashes, and its bit is 0 iff the reverse-complement word is a forward word of the record: flipped,
    except for palindromic words and words present in both orientations (0 on both sides)."""
    flipped = kept = 0
    for seq in records:
        fw = ref.words(seq)
        cvs = sorted({min(f, sref.word_rc(f)) for f in fw}, key=ref.fmix32)
        hashes, bits = sref.sketch(seq, ALL)
        rh, rbits = sref.sketch(sref.rc(seq), ALL)
        assert hashes == [ref.fmix32(cv) for cv in cvs] == rh
        assert bits == [0 if cv in fw else 1 for cv in cvs]
        assert rbits == [0 if sref.word_rc(cv) in fw else 1 for cv in cvs]
        for cv, b, rb in zip(cvs, bits, rbits):
            if sref.word_rc(cv) == cv or (cv in fw and sref.word_rc(cv) in fw):
                assert b == rb == 0
                kept += 1
            else:
                assert b + rb == 1
                flipped += 1
        for s in (16, 100):
            assert sref.sketch(seq, s) == (hashes[:s], bits[:s])
    assert flipped > 100000 and kept > 10
    assert sref.sketch("A" * 500) == ([ref.fmix32(0)], [0]) and sref.sketch("T" * 500) == ([ref.fmix32(0)], [1])
    assert set(sref.sketch("ACGT" * 100)[1]) == {0}            # ACGTACGTACGT and its rotations: CGTA.. / TACG.. are each other's, GTAC.. is its own
    x = rand_seq(random.Random(5), 300)
    assert set(sref.sketch(x + sref.rc(x), ALL)[1]) == {0}
    assert sref.bit_words([1, 0, 1] + [0] * 30 + [1], 40) == [5, 2]


def test_a_root_against_its_own_reverse_complement():
    roots = cases.pair_records()[0::11][:5]
    assert [len(x) for x in roots] == [40, 130, 600, 1500, 3000]
    votes = []
    for x in roots:
        a, b = sref.sketch(x, 1024), sref.sketch(sref.rc(x), 1024)
        same, opp = sref.pair_strand(a, b, 1024)
        assert same + opp == len(a[0]) == min(1024, len({min(f, sref.word_rc(f)) for f in ref.words(x)}))
        assert same == sum(1 for h, bit in zip(*a) if bit == 0 and b[1][b[0].index(h)] == 0)
        assert sref.strand(same, opp) == "-" and sref.strand(*sref.pair_strand(a, a, 1024)) == "+"
        votes.append((same, opp))
    assert votes[3] == (1, 1023)                               # the one shared palindrome counts as same
    x = rand_seq(random.Random(1), 500)
    a, b = sref.sketch(x), sref.sketch(sref.rc(x))
    assert len(a[1]) == 489 and [p + q for p, q in zip(a[1], b[1])] == [1] * 489
    assert sref.strand(0, 0) == "+" and sref.strand(3, 3) == "+" and sref.strand(3, 4) == "-"


def test_forward_sketches_miss_the_reverse_complement():
    """The gap this rule closes, on the forward yardstick: a record against its reverse complement shares only the words it holds in
    both orientations (none in most records) — far below any floor; on canonical sketches it scores as against itself."""
    zero = 0
    for x in cases.pair_records()[0::11][:5]:
        fw = ref.words(x)
        w, u, ani = ref.pair(ref.sketch(x, ALL), ref.sketch(sref.rc(x), ALL), ALL)
        assert w == sum(1 for f in fw if sref.word_rc(f) in fw) and ani < 600000
        if w == 0:
            assert ani == 0
            zero += 1
        a, b = sref.sketch(x, 1024)[0], sref.sketch(sref.rc(x), 1024)[0]
        assert ref.pair(a, b, 1024) == ref.pair(a, a, 1024) == (len(a), len(a), 1000000)
    assert zero >= 3


@pytest.mark.parametrize("s", (16, 100, 1024))
def test_turning_one_side_changes_only_the_vote(s):
    seqs = cases.pair_records()
    sk = [sref.sketch(x, s) for x in seqs]
    rsk = [sref.sketch(sref.rc(x), s) for x in seqs]
    minus = 0
    for a in sk:
        for b, rb in zip(sk, rsk):
            assert ref.pair(a[0], rb[0], s) == ref.pair(a[0], b[0], s)
            same, opp = sref.pair_strand(a, b, s)
            assert same + opp == ref.pair(a[0], b[0], s)[0]
            if ref.pair(a[0], b[0], s)[2] >= 700000:
                assert same > opp and sref.strand(*sref.pair_strand(a, rb, s)) == "-"
                minus += 1
    assert minus > 100
    small = [sk[0], sk[1], sk[12]], [rsk[0], rsk[13]]
    want = [sref.pair_strand(a, b, s) for a in small[0] for b in small[1] if ref.pair(a[0], b[0], s)[2] >= 700000]
    assert sref.groups_strand(*small, s, 700000) == (sum(x for x, _ in want), sum(y for _, y in want))


# ---- the tool, strands injected --------------------------------------------------------------------------------------------------------------
ODD = b">u00 a description, kept\nACGTNryk\nmmAC\n\n>u01\nacgtt\n"       # two lines and an empty one; lower case and IUPAC
ODD_TURNED = b">u00 a description, kept\nGTkkmryNACGT\n>u01\naacgt\n"


@pytest.fixture()
def tree(tmp_path):
    root = str(tmp_path)
    cf = cases.write_tree(root, cases.semantics_clusters())
    for ext in (".fa", ".tfa"):
        open(os.path.join(root, "Clusters_fa", "U_1" + ext), "wb").write(ODD)
    return root, cf, ref.snapshot(root)


def plan(root):
    wd = os.path.join(root, "Clusters_fa")
    i = lambda x: wd + "/" + x
    md = {i("Q_4"): [i("P_2")], i("R_8"): [i("Q_4")], i("L_6"): [i("M_3")], i("E1_3"): [i("U_1")]}
    votes = {(i("Q_4"), i("P_2")): (3, 2000), (i("R_8"), i("Q_4")): (0, 1), (i("L_6"), i("M_3")): (7, 7), (i("E1_3"), i("U_1")): (0, 9)}
    return md, votes


def test_apply_turns_the_minus_merges(tree):
    root, cf, snap = tree
    md, votes = plan(root)
    app = merge_clstr(inputfile=cf, output=os.path.join(root, "history.txt"), threshold=20, drop="F", ani=0.8, both_strands=True, orient=True)
    app.merge_dict = md
    app.strands = {k: (sref.strand(*v),) + v for k, v in votes.items()}
    app.write_history()
    app.write_strands()
    app.apply()
    got = ref.snapshot(root)
    f = lambda name, ext: snap["Clusters_fa/" + name + ext]
    for ext in (".fa", ".tfa"):
        # the chain P(-) -> Q(-) -> R: P lands as it was given (its records are on one line already)
        assert got["Clusters_fa/R_14" + ext] == f("R_8", ext) + sref.rc_fasta(f("Q_4", ext)) + f("P_2", ext)
        assert sref.rc_fasta(sref.rc_fasta(f("P_2", ext))) == f("P_2", ext) != sref.rc_fasta(f("P_2", ext))
        assert got["Clusters_fa/L_9" + ext] == f("L_6", ext) + f("M_3", ext)                  # a tie is +: byte for byte
        assert got["Clusters_fa/E1_4" + ext] == f("E1_3", ext) + ODD_TURNED
    q = ref.read_fasta(os.path.join(root, "Clusters_fa", "R_14.tfa"))[8:12]
    assert q == [(i, sref.rc(s)) for i, s in cases.semantics_clusters()["Q"]]                # headers intact, sequences turned
    assert got["Clusters_fa/R_14.txt"] == f("R_8", ".txt") + f("Q_4", ".txt") + f("P_2", ".txt")
    assert got["Clusters_fa/E1_4.txt"] == f("E1_3", ".txt") + f("U_1", ".txt")
    hist = got["history.txt"].decode().splitlines()
    strand = got["history.txt.strand"].decode().splitlines()
    assert [x.split("\t")[:2] for x in strand] == [x.split("\t") for x in hist] and len(hist) == 4
    assert [x.split("\t")[2:] for x in strand] == [["-", "3", "2000"], ["-", "0", "1"], ["+", "7", "7"], ["-", "0", "9"]]
    assert got["history.txt.strand"].decode() == sref.strand_text(md, votes)
    # the yardstick's file operation on a fresh copy leaves the same tree
    other = root + "_yardstick"
    ref.restore(other, snap)
    md2, votes2 = plan(other)
    clusters = ref.parse_clusters(open(os.path.join(other, "cluster.txt")).read())
    sref.apply_orient(clusters, os.path.join(other, "Clusters_fa"), md2, {k: sref.strand(*v) for k, v in votes2.items()})
    want = ref.snapshot(other)
    assert {k: v for k, v in got.items() if not k.startswith("history")} == want


def test_without_orient_the_strands_change_no_file(tree):
    root, cf, snap = tree
    md, votes = plan(root)
    app = merge_clstr(inputfile=cf, output=os.path.join(root, "history.txt"), threshold=20, drop="F", ani=0.8, both_strands=True)
    app.merge_dict = md
    app.strands = {k: (sref.strand(*v),) + v for k, v in votes.items()}
    app.apply()
    other = root + "_forward"
    ref.restore(other, snap)
    md2, _ = plan(other)
    ref.apply(ref.parse_clusters(open(os.path.join(other, "cluster.txt")).read()), os.path.join(other, "Clusters_fa"), md2, "F")
    assert ref.snapshot(root) == ref.snapshot(other)


def test_orient_is_refused_without_both_strands_or_with_drop(tree):
    root, cf, snap = tree

    def run(*extra):
        return subprocess.run([sys.executable, SCRIPT, "-i", "cluster.txt", "-t", "20", "-o", "history.txt", "-a", "0.8"] + list(extra),
                              cwd=root, capture_output=True, text=True, timeout=120)
    for flags in (("--orient", "-d", "F"), ("--orient",), ("--both-strands", "--orient", "-d", "T"), ("--both-strands", "--orient")):
        res = run(*flags)
        assert res.returncode == 2 and "--orient" in res.stderr, flags
        assert ref.snapshot(root) == snap
    for kw in (dict(orient=True, drop="F"), dict(orient=True, both_strands=True, drop="T")):
        with pytest.raises(ValueError, match="orient"):
            merge_clstr(inputfile=cf, **kw)
