"""Inputs of the identity-merge tests (tests/test_ani.py checks what they are meant to provoke on the yardstick alone,
tests/test_ani_gpu.py compares the device with the yardstick on them).  A helper, not a test."""
import os
import random

from anchor_cases import rand_seq, substitute

SKETCH_SIZES = (16, 64, 100, 1024)
SORT_SIZES = (256, 2048, 8192, 16384)          # word counts at which the sketch kernel changes its sort size (below the last, 32768)


def sketch_records(seed=11):
    """[(label, sequence)]: the shapes of the sketch comparison.  `words s-1` etc. are random records of that many word positions (all
    distinct: tests/test_ani.py counts them) for every sketch size tested."""
    rng = random.Random(seed)
    out = [("len %d" % n, rand_seq(rng, n)) for n in (8, 11, 12, 13, 1035)]
    for s in SKETCH_SIZES:
        out += [("words %d%+d" % (s, d), rand_seq(rng, s + d + 11)) for d in (-1, 0, 1)]
    out.append(("500 x A", "A" * 500))
    out.append(("tandem repeat", "ACGGTCATTG" * 70 + "ACG"))
    n10 = list(rand_seq(rng, 400))
    n10[::10] = "N" * len(n10[::10])
    out.append(("N every 10 bases", "".join(n10)))
    mid = rand_seq(rng, 300)
    out.append(("one N in the middle", mid[:150] + "N" + mid[151:]))
    out.append(("lower case", rand_seq(rng, 700).lower()))
    for n in SORT_SIZES:
        out += [("sort size %d%+d" % (n, d), rand_seq(rng, n + d + 11)) for d in (-1, 0, 1)]
    out.append(("32767 bases", rand_seq(rng, 32767)))
    out.append(("empty", ""))
    return out


def pair_records(seed=12):
    """About 60 records for the all-ordered-pairs comparison: five families at 0 .. 30 % substitutions of roots of 40 .. 3000 bases, some
    truncated; empty-sketch records; at s = 16 / 100 / 1024 full sketches meet non-full ones and non-full ones each other."""
    rng = random.Random(seed)
    out = []
    for f, n in enumerate((40, 130, 600, 1500, 3000)):
        root = rand_seq(rng, n)
        out.append(root)
        for k, rate in enumerate((0.0, 0.02, 0.05, 0.08, 0.1, 0.12, 0.15, 0.2, 0.25, 0.3)):
            s = substitute(rng, root, int(rate * n))
            if k % 3 == 2:
                cut = rng.randint(0, n // 4)
                s = s[cut:n - rng.randint(0, n // 4)]
            out.append(s.lower() if k == 4 else s)
    out += ["", "ACGTACGTACG", "N" * 50, "ACGTNACGTNACGTNACGTNACGTN", rand_seq(rng, 12)]
    return out


def group_records(seed=13):
    """(records, groups): 24 distinct short records (three families of seven at 0 .. 25 % and three without a word) and groups as lists
    of record numbers — 1, 63, 64, 65 and 500 members (records reused), one of empty sketches only, one unrelated to the others."""
    rng = random.Random(seed)
    records = []
    for n in (90, 140, 200):
        root = rand_seq(rng, n)
        records += [root] + [substitute(rng, root, int(rate * n)) for rate in (0.0, 0.03, 0.06, 0.1, 0.15, 0.25)]
    records += ["", "ACGTACG", "N" * 40]
    groups = [[3],
              [rng.randrange(0, 14) for _ in range(63)],
              [rng.randrange(7, 21) for _ in range(64)],
              [rng.randrange(0, 24) for _ in range(65)],
              [rng.randrange(0, 24) for _ in range(500)],
              [21, 22, 23, 21, 22],
              [14, 15, 16, 17, 18, 19, 20, 14]]      # the third family only: nothing reported against groups[0]
    return records, groups


# ---- Clusters_fa trees -------------------------------------------------------------------------------------------------------------------
def members(rng, root, n, prefix):
    """n records at 0 .. 3 % of root."""
    return [(">%s%02d" % (prefix, k), root if k == 0 else substitute(rng, root, rng.randint(0, int(0.03 * len(root))))) for k in range(n)]


def golden_clusters(seed=21, n=600):
    """[[(id, sequence)]] in .clstr order, about 10 clusters, no chain: three large unrelated clusters and rare ones — at 10-12 % of a
    large root (merge), at 22 % (reported, below 0.8), unrelated (stay), three of one member (ties in size)."""
    rng = random.Random(seed)
    b1, b2, b3 = rand_seq(rng, n), rand_seq(rng, n), rand_seq(rng, n)
    return [members(rng, b1, 6, "ba"),
            members(rng, substitute(rng, b1, int(0.10 * n)), 3, "ra"),
            members(rng, b2, 5, "bb"),
            members(rng, rand_seq(rng, n), 1, "ua"),
            members(rng, substitute(rng, b2, int(0.12 * n)), 2, "rb"),
            members(rng, b3, 4, "bc"),
            members(rng, substitute(rng, b3, int(0.11 * n)), 1, "rc"),
            members(rng, substitute(rng, b1, int(0.22 * n)), 2, "rd"),
            members(rng, rand_seq(rng, n), 2, "ub"),
            members(rng, substitute(rng, b3, int(0.10 * n)), 1, "re")]


GOLDEN_FLAGS = dict(t=3, a=0.7)


def semantics_clusters(seed=22, n=1500):
    """Named clusters for the -a / -t / chain tests: R (8) <- Q (4, 11 % of R) <- P (2, 11 % of Q, so about 21 % of R): a chain;
    L (6, unrelated) <- M (3, 22 % of L: reported but below 0.8); E1, E2 (3 each, 5 % apart: equal sizes, never compared); U (1,
    unrelated)."""
    rng = random.Random(seed)
    r, l, e = rand_seq(rng, n), rand_seq(rng, n), rand_seq(rng, n)
    q = substitute(rng, r, int(0.11 * n))
    p = substitute(rng, q, int(0.11 * n))
    return {"R": members(rng, r, 8, "r"), "L": members(rng, l, 6, "l"), "Q": members(rng, q, 4, "q"),
            "E1": members(rng, e, 3, "ea"), "M": members(rng, substitute(rng, l, int(0.22 * n)), 3, "m"),
            "E2": members(rng, substitute(rng, e, int(0.05 * n)), 3, "eb"), "P": members(rng, p, 2, "p"),
            "U": members(rng, rand_seq(rng, n), 1, "u")}


def write_tree(root, named):
    """The tree extract_cluster.py leaves for {name: [(id, sequence)]}: root/cluster.txt and root/Clusters_fa/name_size.fa, .tfa, .txt
    and name_size/<id>.fa.  Returns the path of cluster.txt."""
    wd = os.path.join(root, "Clusters_fa")
    os.makedirs(wd)
    with open(os.path.join(root, "cluster.txt"), "w") as f:
        f.write("#Cluster_id\tNumber\n")
        for name, recs in named.items():
            f.write("%s\t%d\n" % (name, len(recs)))
    for name, recs in named.items():
        stem = "%s_%d" % (name, len(recs))
        os.makedirs(os.path.join(wd, stem))
        text = "".join("%s\n%s\n" % (i, s) for i, s in recs)
        for ext in (".fa", ".tfa"):
            open(os.path.join(wd, stem + ext), "w").write(text)
        with open(os.path.join(wd, stem + ".txt"), "w") as f:
            for i, s in recs:
                f.write("Clusters_fa/%s/%s.fa\n" % (stem, i[1:]))
                open(os.path.join(wd, stem, i[1:] + ".fa"), "w").write("%s\n%s\n" % (i, s))
    return os.path.join(root, "cluster.txt")
