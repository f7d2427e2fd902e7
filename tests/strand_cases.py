"""Inputs of the both-strand tests (tests/test_strand.py checks what they are meant to provoke on the yardstick alone,
tests/test_strand_gpu.py compares the device with the yardstick on them).  A helper, not a test.  Built on anchor_cases, star_cases and
cluster_cases, whose constructions are reused with some records replaced by their reverse complements."""
import random

import anchor_cases
import cluster_cases
import star_cases
import strand_ref as ref
from anchor_cases import rand_seq, substitute

LENGTHS = (1, 11, 12, 13, 63, 64, 65, 127, 128, 129)


def agroup(name, anchor, queries, planted, **kw):
    """anchor_cases.group plus `planted`: which queries were replaced by their reverse complement."""
    return dict(anchor_cases.group(name, anchor, queries, **kw), planted=list(planted))


def turn_some(records, which):
    """The records with those picked by which(index) replaced by their reverse complement, and the list of the picked."""
    turned = [bool(which(q)) for q in range(len(records))]
    return [ref.rc(r) if t else r for r, t in zip(records, turned)], turned


# ---- anchored alignment: one anchor of 300 bases ----------------------------------------------------------------------------------------
def anchor_300():
    """300 bases holding a 40-base stretch that is its own reverse complement at 130 .. 170."""
    rng = random.Random(41)
    half = rand_seq(rng, 20)
    return rand_seq(rng, 130) + half + ref.rc(half) + rand_seq(rng, 130)


def tie_queries(a):
    """Queries whose two strands draw: the self-complementary stretch (its rc is itself), and a query made of a[10:30] and
    rc(a[200:220]) around a spacer that shares no word with either strand — nine votes on one diagonal each way."""
    return [a[130:170], a[10:30] + "N" * 5 + ref.rc(a[200:220])]


def anchor_groups():
    a = anchor_300()
    rng = random.Random(43)
    out = []
    # a random family, every second query turned
    qs = []
    for _ in range(60):
        m = rng.randint(40, 110)
        a0 = rng.randint(0, 130 - m) + rng.choice((0, 170))        # (beside the self-complementary stretch, which votes both ways)
        q = list(substitute(rng, a[a0:a0 + m], rng.randint(0, 4)))
        if rng.random() < 0.5:
            p, g = rng.randint(5, m - 5), rng.randint(1, 4)
            if rng.random() < 0.5:
                del q[p:p + g]
            else:
                q[p:p] = list(rand_seq(rng, g))
        qs.append("".join(q))
    qs, turned = turn_some(qs, lambda q: q % 2 == 1)
    out.append(agroup("family-half-turned", a, qs, turned))
    # lengths around the vote word, the wavefront and the lane stride of the in-place swap (pairs x, m - 1 - x: 64 to a pass), each
    # length once as given and once turned; under 12 bases nothing votes and nothing is turned
    qs, planted = [], []
    for m in LENGTHS:
        s = rng.randint(0, 130 - m)
        qs += [a[s:s + m], ref.rc(a[s:s + m])]
        planted += [False, m >= 12]
    out.append(agroup("lengths", a, qs, planted))
    out.append(agroup("draws", a, tie_queries(a), [False, False]))
    # IUPAC letters, lower case and U in a turned query (U becomes A), and the same letters in one left as given
    seg = list(a[30:128])
    for p, ch in ((5, "R"), (6, "Y"), (20, "K"), (21, "M"), (40, "B"), (41, "V"), (60, "D"), (61, "H"), (75, "S"), (76, "W"), (80, "N"),
                  (90, "U"), (91, "u"), (93, "*")):
        seg[p] = ch
    seg = "".join(seg)
    mixed = "".join(ch.lower() if k % 3 == 0 else ch for k, ch in enumerate(seg))
    out.append(agroup("letters", a, [ref.rc(mixed).lower(), mixed, ref.rc(seg)], [True, False, True]))
    # a query longer than the anchor
    out.append(agroup("longer", a, [ref.rc(rand_seq(rng, 17) + a + rand_seq(rng, 23)), rand_seq(rng, 17) + a + rand_seq(rng, 23)], [True, False]))
    return out


def long_group():
    """One turned query of the length limit at band 4: the vote histogram takes (32767 + 300) / 2 + 1 words of LDS.  No band of an anchor
    of 300 reaches row 32767, so the record comes back turned, with its d0 and without a path."""
    a = anchor_300()
    rng = random.Random(53)
    q = rand_seq(rng, 20000) + a[20:280] + rand_seq(rng, 32767 - 20000 - 260)
    return agroup("limit", a, [ref.rc(q)], [True], band=4)


def anchor_yardstick(g, strands=True):
    align = ref.align if strands else anchor_cases.ref.align
    return [align(q, g["anchor"], g["col"], g["width"], **g["params"]) for q in g["queries"]]


# ---- star alignment ---------------------------------------------------------------------------------------------------------------------
def star_groups():
    out = []
    g = star_cases.planted_family(1)
    recs, turned = turn_some(star_cases.cleaned(g), lambda q: q % 3 == 1)
    out.append(star_cases.group("family-third-turned", recs, planted=turned))
    # the drifting record (its path touches the band at W = 32 and is aligned again at 64) turned
    g = [x for x in star_cases.drift_groups() if x["name"] == "drift-64-ins"][0]
    recs, turned = turn_some(star_cases.cleaned(g), lambda q: q == 1)
    out.append(star_cases.group("drift-turned", recs, planted=turned))
    # three rounds against a moving consensus
    g = [x for x in star_cases.consensus_groups() if x["name"] == "consensus-moves"][0]
    recs, turned = turn_some(star_cases.cleaned(g), lambda q: q in (2, 3, 6))
    out.append(star_cases.group("consensus-turned", recs, rounds=3, planted=turned))
    return out


def star_yardstick(g):
    return ref.star(g["records"], rounds=g["rounds"], **g["params"])


# ---- clustering -------------------------------------------------------------------------------------------------------------------------
def pair_set(seed=59):
    """20 records: two families of the lengths above cut from a root of 210 bases, every second one turned."""
    rng = random.Random(seed)
    seqs = []
    for f in range(2):
        root = rand_seq(rng, 210)
        for k, m in enumerate(LENGTHS):
            s0 = rng.randint(0, 210 - m)
            s = root[s0:s0 + m]
            if m >= 63:
                s = cluster_cases.mutate(rng, s, rng.randint(0, m // 12), k % 3)
            if m == 129:
                s = s[:40] + "N" + s[41:]
            seqs.append(ref.rc(s) if (k + f) % 2 else s)
    return seqs


def family_set(seed=61, n_families=6, per_family=8):
    """Families of a root of 150 .. 400 bases, members at 2 .. 21 % substitutions (both sides of 0.8 and 0.9) and exact copies and
    substrings (for 1.0), every second member turned; shuffled."""
    rng = random.Random(seed)
    seqs = []
    for f in range(n_families):
        root = rand_seq(rng, rng.randint(185, 390))
        fam = [root, root[5:len(root) - 7], root]
        while len(fam) < per_family:
            rate = rng.choice((0.02, 0.05, 0.09, 0.11, 0.15, 0.19, 0.21))
            s = cluster_cases.mutate(rng, root, int(rate * len(root)), rng.randint(0, 2))
            fam.append(s[rng.randint(0, 20):] if len(s) > 170 else s)
        seqs += [ref.rc(s) if k % 2 else s for k, s in enumerate(fam)]
    rng.shuffle(seqs)
    return seqs


def edge_set(seed=67):
    """Records under 12 bases (no vote either way: each founds its own cluster), a 12-mer that joins turned, and a record with N, which
    never matches: at 1.0 it founds its own cluster on either strand."""
    rng = random.Random(seed)
    e = rand_seq(rng, 90)
    return [e, ref.rc(e), ref.rc(e[:40] + "N" + e[41:]), e[:40] + "N" + e[41:], e[5:16], ref.rc(e[5:16]), ref.rc(e[20:32]), e[50:62],
            ref.rc(e[3:80]).lower()]


def mixed_set(seed=71):
    """About 30 named records for the scripts end to end: three families of ten, every second member turned, input order shuffled."""
    rng = random.Random(seed)
    seqs = []
    for f in range(3):
        root = rand_seq(rng, (180, 240, 300)[f])
        fam = [root] + [cluster_cases.mutate(rng, root, rng.randint(2, len(root) // 9), rng.randint(0, 2))[rng.randint(0, 6):] for _ in range(9)]
        seqs += [ref.rc(s) if k % 2 else s for k, s in enumerate(fam)]
    rng.shuffle(seqs)
    return cluster_cases.named(seqs, "m")
