"""The yardstick of clustering by identity (tests/cluster_ref.py) against invariants that do not come from it, on the cases of
tests/cluster_cases.py, and the .clstr layout against what the reference's extract_cluster reads from it (tests/golden/cluster_small.*,
tests/golden/make_golden_cluster.py).  No GPU."""
import gzip
import os

import pytest

import cluster_cases as cases
import cluster_ref as ref
from conftest import GOLDEN

ACGT = "ACGT"


@pytest.fixture(scope="module")
def special():
    records = cases.special()
    ids, seqs = [i for i, _ in records], [s.upper() for _, s in records]
    memo = {}
    return ids, seqs, {p: ref.cluster(seqs, memo=memo, identity_permille=p) for p in (800, 1000)}


def most_matches(s, r):
    """The largest number of equal A/C/G/T pairs ANY alignment of s and r can hold (a longest common subsequence over those letters):
    exhaustive, no band, no scores — an upper bound of every n_match the rule can report."""
    prev = [0] * (len(r) + 1)
    for x in s:
        cur = [0]
        for j, y in enumerate(r):
            cur.append(max(prev[j + 1], cur[j], prev[j] + (x == y and x in ACGT)))
        prev = cur
    return prev[-1]


@pytest.mark.parametrize("permille", (800, 1000))
def test_members_meet_the_threshold_and_representatives_do_not(permille, special):
    ids, seqs, res = special
    cluster_of, reps, n_match_of = res[permille]
    assert sorted(set(cluster_of)) == list(range(len(reps))) and [cluster_of[r] for r in reps] == list(range(len(reps)))
    # creation order is length descending, ties by input order
    assert [(-len(seqs[r]), r) for r in reps] == sorted((-len(seqs[r]), r) for r in reps)
    for i, k in enumerate(cluster_of):
        r = reps[k]
        if i == r:
            continue
        assert len(seqs[i]) <= len(seqs[r]) and (len(seqs[i]), -i) < (len(seqs[r]), -r)
        assert n_match_of[i] * 1000 >= permille * len(seqs[i])
        assert most_matches(seqs[i], seqs[r]) >= n_match_of[i]
    # no representative is similar to an earlier one; a member is similar to no representative before its own
    for a, r in enumerate(reps):
        for e in reps[:a]:
            assert ref.similar(seqs[r], seqs[e], identity_permille=permille) is None
    for i, k in enumerate(cluster_of):
        for e in reps[:k]:
            if (len(seqs[e]), -e) > (len(seqs[i]), -i):
                assert ref.similar(seqs[i], seqs[e], identity_permille=permille) is None


def test_the_named_situations(special):
    ids, seqs, res = special
    c8, reps8, nm8 = res[800]
    c10, reps10, _ = res[1000]
    # equal lengths: the earlier record founds the cluster
    assert reps8[c8[0]] == 0 and c8[1] == c8[0] and c8[2] == c8[0]
    # similar to two representatives: the earlier-created one (the longer) takes it
    assert reps8[c8[3]] == 3 and reps8[c8[4]] == 4 and c8[5] == c8[3]
    assert ref.similar(seqs[5], seqs[4]) is not None
    # the chain: b joins a, c is similar to b but not to a and founds its own cluster
    assert c8[7] == c8[6] and reps8[c8[8]] == 8 and ref.similar(seqs[8], seqs[7]) is not None and ref.similar(seqs[8], seqs[6]) is None
    # duplicates, substrings and the lower-case copy collapse at 1.0; one substitution does not
    assert len({c10[i] for i in range(9, 15)}) == 1 and reps10[c10[9]] == 9 and c10[15] != c10[9] and c8[15] == c8[9]
    # N never matches: at 1.0 the records with N stand alone, at 0.8 they join
    assert c10[17] != c10[16] and c10[18] != c10[16] and c8[17] == c8[16] and c8[18] == c8[16] and reps8[c8[19]] == 19
    # 11 bases cast no vote; 12 do
    assert reps8[c8[21]] == 21 and c8[22] == c8[20] and reps8[c8[23]] == 23 and c8[24] == c8[20]
    assert reps8[c8[25]] == 25 and reps8[c8[26]] == 26 and c8[27] == c8[26]
    # lower case is upper-cased
    assert c8[29] == c8[28] and c8[30] == c8[28] and nm8[29] == 106
    # the threshold is inclusive: 80 of 100 joins at 0.8, 79 does not
    assert c8[32] == c8[31] and nm8[32] == 80 and reps8[c8[33]] == 33 and c8[34] == c8[31] and nm8[34] == 90


def test_identity_text_is_integer_rounding():
    assert ref.identity_text(80, 100) == "80.00%" and ref.identity_text(2, 3) == "66.67%" and ref.identity_text(1, 3) == "33.33%"
    assert ref.identity_text(399, 400) == "99.75%" and ref.identity_text(1, 8) == "12.50%" and ref.identity_text(5, 5) == "100.00%"
    from multiprime_amd.cluster import identity_text
    assert all(identity_text(a, m) == ref.identity_text(a, m) for m in (1, 3, 7, 64, 399) for a in range(m + 1))


def test_clstr_round_trip(special):
    ids, seqs, res = special
    cluster_of, reps, n_match_of = res[800]
    text = ref.clstr_text(ids, seqs, cluster_of, reps, n_match_of)
    parsed = ref.parse_clstr(text)
    assert len(parsed) == len(reps) and sum(len(c) for c in parsed) == len(ids)
    seen = []
    for k, members in enumerate(parsed):
        assert [m[0] for m in members] == list(range(len(members)))
        assert [m[2] for m in members if m[3] == "*"] == [ids[reps[k]]]
        for num, length, ident, tail in members:
            i = ids.index(ident)
            seen.append(i)
            assert cluster_of[i] == k and length == len(seqs[i])
            assert tail == ("*" if i == reps[k] else ref.identity_text(n_match_of[i], length))
        assert [ids.index(m[2]) for m in members] == sorted(ids.index(m[2]) for m in members)
    assert sorted(seen) == list(range(len(ids)))


def golden(name):
    with gzip.open(os.path.join(GOLDEN, name), "rt") as f:
        return f.read()


def test_the_reference_reads_our_clstr():
    fa, clstr = golden("cluster_small.fa.gz"), golden("cluster_small.clstr.gz")
    ids, seqs = zip(*ref.read_fasta(fa))
    assert [(i, s) for i, s in zip(ids, seqs)] == [(i, s.upper()) for i, s in cases.special()]
    assert ref.clstr_text(ids, seqs, *ref.cluster(list(seqs), identity_permille=800)) == clstr
    parsed = ref.parse_clstr(clstr)
    # cluster.txt: the reference's member count per cluster; cluster.identities.txt: cluster, id, identity of every non-representative
    txt = golden("cluster_small.txt.gz").splitlines()
    assert txt[0] == "#Cluster_id\tNumber" and txt[1:] == ["Cluster_%d\t%d" % (k, len(m)) for k, m in enumerate(parsed)]
    want = ["Cluster_%d\t%s\t%s" % (k, ident[1:], tail) for k, m in enumerate(parsed) for _, _, ident, tail in m if tail != "*"]
    assert golden("cluster_small.identities.txt.gz").splitlines() == want and len(want) > 50
