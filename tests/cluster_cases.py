"""Inputs of the clustering tests (tests/test_cluster.py checks what they are meant to provoke on the yardstick alone,
tests/test_cluster_gpu.py compares the device with the yardstick on them).  A helper, not a test.  Every case is a list of
(id, sequence) in input order; ids carry '>' as the FASTA front end returns them."""
import random

from anchor_cases import rand_seq, substitute


def mutate(rng, s, n_sub, n_indel=0):
    """n_sub substitutions, then n_indel indels of 1..3 bases away from the ends."""
    s = list(substitute(rng, s, n_sub))
    for _ in range(n_indel):
        p, g = rng.randint(8, len(s) - 8), rng.randint(1, 3)
        if rng.random() < 0.5:
            del s[p:p + g]
        else:
            s[p:p] = list(rand_seq(rng, g))
    return "".join(s)


def named(seqs, prefix="s"):
    return [(">%s%04d" % (prefix, i), s) for i, s in enumerate(seqs)]


def families(seed=1, n_families=12, per_family=12):
    """Planted families: members at 2 .. 30 % substitutions of a root of 40 .. 400 bases (both sides of 0.8 and 0.9), some with indels,
    some truncated; shuffled, so that length order and input order differ."""
    rng = random.Random(seed)
    seqs = []
    for f in range(n_families):
        root = rand_seq(rng, rng.choice((40, 64, 90, 128, 150, 200, 260, 400)))
        seqs.append(root)
        for k in range(per_family - 1):
            rate = rng.choice((0.02, 0.05, 0.09, 0.11, 0.15, 0.19, 0.21, 0.3))
            s = mutate(rng, root, int(rate * len(root)), rng.randint(0, 2) if len(root) >= 64 else 0)
            if k % 4 == 0 and len(s) > 60:
                cut = rng.randint(0, len(s) // 4)
                s = s[cut:len(s) - rng.randint(0, len(s) // 4)]
            seqs.append(s)
    rng.shuffle(seqs)
    return named(seqs, "f")


def special(seed=2):
    """The named situations of the rule, beside a few unrelated records."""
    rng = random.Random(seed)
    seqs = []
    # equal lengths: the earlier record in the input founds the cluster
    a = rand_seq(rng, 120)
    seqs += [substitute(rng, a, 3), a, substitute(rng, a, 5)]
    # a member similar to two representatives joins the earlier-created (the longer one; then the earlier in the input)
    left, mid, right = rand_seq(rng, 100), rand_seq(rng, 100), rand_seq(rng, 100)
    seqs += [left + mid + rand_seq(rng, 40), rand_seq(rng, 30) + mid + right, mid]
    # a chain: b is similar to a, c to b, c not to a (substitutions pile up) — c founds its own cluster
    ca = rand_seq(rng, 200)
    cb = substitute(rng, ca, 30, 0, 100)
    cc = substitute(rng, cb, 30, 100, 200)
    seqs += [ca + "A", cb, cc[:-1]]
    # exact substrings and exact duplicates: one cluster at identity 1.0
    d = rand_seq(rng, 150)
    seqs += [d, d, d[10:140], d[:80], d[70:], d.lower(), d[:149] + ("A" if d[149] != "A" else "C")]
    # N: never a match — at 1.0 the record with N founds its own cluster
    e = rand_seq(rng, 90)
    seqs += [e, e[:40] + "N" + e[41:], e[:20] + "NNNNN" + e[25:], "N" * 50]
    # 11 bases cast no vote, 12 do
    g = rand_seq(rng, 60)
    seqs += [g, g[5:16], g[5:17], g[20:31].lower(), g[20:32].lower(), "ACGTACGTACG", "ACGTACGTACGT", "ACGTACGTACGT"]
    # lower case, mixed case
    h = rand_seq(rng, 110)
    seqs += [h.lower(), substitute(rng, h, 4), "".join(ch.lower() if k % 3 else ch for k, ch in enumerate(substitute(rng, h, 8)))]
    # around the threshold: 100 bases with exactly 80 / 79 / 90 / 89 matches against the first
    t = rand_seq(rng, 100) + rand_seq(rng, 30)
    seqs += [t] + [substitute(rng, t[:100], k, 14, 86) for k in (20, 21, 10, 11)]
    seqs += [rand_seq(rng, n) for n in (40, 41, 77, 130, 300, 399, 400)]
    # small families to fill the rounds of a small block
    for _ in range(8):
        root = rand_seq(rng, rng.randint(60, 180))
        seqs += [root] + [mutate(rng, root, rng.randint(1, len(root) // 6), rng.randint(0, 1)) for _ in range(7)]
    return named(seqs, "x")


def pair_case(seed=3):
    """About 60 records in five families, lengths around the vote word and the wavefront (8, 11, 12, 13, 63, 64, 65, 127, 128, 129),
    for the all-ordered-pairs comparison."""
    rng = random.Random(seed)
    seqs = []
    for f in range(5):
        root = rand_seq(rng, 210)
        lengths = (210, 8, 11, 12, 13, 63, 64, 65, 127, 128, 129, 170)
        for k, m in enumerate(lengths):
            s0 = rng.randint(0, 210 - m)
            s = root[s0:s0 + m]
            if m >= 63:
                s = mutate(rng, s, rng.randint(0, m // 12), k % 3)
            if m == 129:
                s = s[:40] + "N" + s[41:]
            seqs.append(s.lower() if k == 6 else s)
    return named(seqs, "p")


def all_cases():
    return {"families": families(), "special": special()}


def fasta(records, width=0):
    return "".join("%s some description\n%s\n" % (i, s) for i, s in records)
