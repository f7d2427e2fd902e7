"""Inputs of the anchored-alignment tests (tests/test_anchor.py checks what they are meant to provoke on the yardstick alone,
tests/test_anchor_gpu.py compares the device with the yardstick on them).  A helper, not a test.  Every group is one anchor, one
parameter set and a list of queries; col spreads the anchor over a wider seed so that the column map is exercised."""
import random

import anchor_ref as ref


def rand_seq(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def substitute(rng, s, k, lo=0, hi=None):
    s = list(s)
    for p in rng.sample(range(lo, hi if hi is not None else len(s)), k):
        s[p] = rng.choice([b for b in "ACGT" if b != s[p]])
    return "".join(s)


def group(name, anchor, queries, band=32, match=5, mismatch=4, gap_open=10, gap_extend=2, min_identity_permille=500):
    n = len(anchor)
    col = [2 * j + 1 + (j > n // 2) for j in range(n)]
    return dict(name=name, anchor=anchor, col=col, width=2 * n + 5, queries=list(queries),
                params=dict(band=band, match=match, mismatch=mismatch, gap_open=gap_open, gap_extend=gap_extend,
                            min_identity_permille=min_identity_permille))


def planted_indel(W, g, kind, seed=0):
    """(anchor, query) with one gap of g bases behind a long matching head (it wins the vote: d0 = 0), followed by a run of A.  The
    gap's own bases hold no A, so the only good alignment takes the whole gap at once.  With g <= W it fits the band; with g = W + 1
    the best banded path takes W of them along the band's edge and pairs the last base of the gap, a C, against an A: it scores less
    than the unbanded optimum and touches the edge."""
    rng = random.Random(1000 * W + 10 * g + seed)
    h, r = (100, 30) if W < 50 else (160, 60)
    head = rand_seq(rng, h - 1) + "G"
    filler = rand_seq(rng, g - 1, "CGT") + "C"
    mutated = substitute(rng, head, 3, 5, h - 10)
    # (W = 0 has no edge diagonal beside d0 to run along: there the gap is followed by random bases instead, which only the gap aligns)
    run = "A" * (r + 10) if W else rand_seq(rng, r + 10)
    if kind == "del":
        return head + filler + run + rand_seq(rng, 20, "CGT"), mutated + run[:r]
    return head + run + rand_seq(rng, 20, "CGT"), mutated + filler + run[:r]


def band_gaps(W):
    return sorted({g for g in (1, 2, W - 1, W, W + 1) if g >= 1})


BANDS = (0, 1, 31, 32, 33, 100)


def band_groups():
    out = []
    for W in BANDS:
        for g in band_gaps(W):
            for kind in ("del", "ins"):
                anchor, query = planted_indel(W, g, kind)
                # (W = 1: under the default scores two mismatches beat a one-base gap plus one mismatch, and the best path would not leave
                # d0 at all; a cheaper gap opening restores the case)
                out.append(group(f"band{W}-{kind}{g}", anchor, [query], band=W, gap_open=2 if W == 1 else 10))
    return out


def random_set(n_queries=200, seed=7):
    """Queries mutated from one 257-base anchor: 3 % substitutions, up to two short indels — most paths stay inside W = 32."""
    rng = random.Random(seed)
    anchor = rand_seq(rng, 257)
    queries = []
    for _ in range(n_queries):
        m = rng.randint(40, 110)
        a0 = rng.randint(0, len(anchor) - m)
        q = list(anchor[a0:a0 + m])
        for p in range(len(q)):
            if rng.random() < 0.03:
                q[p] = rng.choice("ACGT")
        for _ in range(rng.randint(0, 2)):
            p, g = rng.randint(5, len(q) - 5), rng.randint(1, 4)
            if rng.random() < 0.5:
                del q[p:p + g]
            else:
                q[p:p] = list(rand_seq(rng, g))
        queries.append("".join(q))
    return group("random200", anchor, queries)


def identity_boundary():
    """A 100-base query with exactly 90 matching pairs: accepted at 900 permille, rejected at 901."""
    rng = random.Random(11)
    anchor = rand_seq(rng, 140)
    query = substitute(rng, anchor[20:120], 10, 15, 85)
    return [group("identity900", anchor, [query], min_identity_permille=900), group("identity901", anchor, [query], min_identity_permille=901)]


def tie_groups():
    rng = random.Random(5)
    a = rand_seq(rng, 30) + "A" * 20 + rand_seq(rng, 30) + "CA" * 12 + rand_seq(rng, 30)
    qs = []
    for run in (17, 18, 19, 21, 23):                     # the run of A shorter / longer than the anchor's 20
        qs.append(a[:30] + "A" * run + a[50:80])
    for rep in (9, 10, 11, 13, 14):                      # the CA repeat shorter / longer than the anchor's 12
        qs.append(a[50:80] + "CA" * rep + a[104:])
    qs += ["A" * 15, "A" * 25, "CA" * 8, "ACAC" * 7, a[20:60]]
    out = [group("ties", a, qs), group("ties-open0", a, qs, gap_open=0), group("ties-flat", a, qs, match=1, mismatch=1, gap_open=0, gap_extend=1)]
    # one 12-mer twice in the anchor (positions 4 and 40), once in the query at 22: diagonals -18 and +18 with one vote each
    k = "ACGTTGCAAGCT"
    a2 = rand_seq(rng, 4, "CT") + k + "CTCTTCTCCTTCTCTCCTCTTTCC" + k + "TCCTCTTCCT"
    q2 = "GAGAGGAGAAGGAGAGGAGAAG" + k + "GGAGA"
    assert a2.index(k) == 4 and a2.index(k, 5) == 40 and q2.index(k) == 22
    out.append(group("vote-tie", a2, [q2, k, k + k], band=24))
    return out


def shape_groups():
    rng = random.Random(3)
    a = rand_seq(rng, 257)
    out = []
    # query lengths around the vote word and the wavefront
    qs = []
    for m in (1, 11, 12, 13, 63, 64, 65, 129):
        s = rng.randint(0, 257 - m)
        qs.append(a[s:s + m])
        if m > 20:
            qs.append(substitute(rng, a[s:s + m], 3))
    out.append(group("lengths", a, qs))
    for n in (12, 64, 65):
        an = rand_seq(rng, n)
        qs = [an, an[: n // 2 + 3], an[n // 3:], rand_seq(rng, 5) + an + rand_seq(rng, 6), substitute(rng, an, 2), an[:6] + an[8:]]
        out.append(group(f"anchor{n}", an, qs))
    # query ends: an insertion at the first / last base, a fragment of the middle, an overhang on both sides
    qs = ["G" + a[:80], a[257 - 80:] + "T", "G" + a[:60] + "T", a[100:160], rand_seq(rng, 7) + a + rand_seq(rng, 9),
          rand_seq(rng, 5) + a[:50]]
    out.append(group("ends", a, qs))
    out.append(group("no-path", a, [rand_seq(rng, 5) + a[:50], a[:40]], band=2))
    # letters
    q = a[40:140]
    qn = list(q)
    for p, ch in ((3, "N"), (17, "R"), (18, "Y"), (50, "n"), (51, "k"), (99, "W")):
        qn[p] = ch
    out.append(group("letters", a, [q.lower(), "".join(qn), "".join(qn).lower(), "N" * 30, "acgtn" * 6]))
    an = list(a)
    for p in (0, 60, 61, 62, 130, 256):
        an[p] = "N"
    an = "".join(an)
    out.append(group("anchor-N", an, [a[40:140], a[:70], a[200:], an[50:75]]))
    # substitutions only
    out.append(group("subs", a, [substitute(rng, a[s:s + 120], k) for s, k in ((0, 1), (30, 5), (100, 12), (137, 30))]))
    # unrelated queries: uniform random ones (under the default scores a banded alignment still pairs over half of their bases with
    # equal ones, so they pass min_identity 0.5) and random ones of another composition (A/G against a C/T anchor: rejected)
    out.append(group("unrelated", a, [rand_seq(rng, 90), rand_seq(rng, 40), rand_seq(rng, 13)]))
    out.append(group("rejected", rand_seq(rng, 130, "CT"), [rand_seq(rng, 90, "AG"), rand_seq(rng, 30, "AG"), rand_seq(rng, 12, "AG")]))
    # several diagonals per lane: 2, 4 and 8
    for W in (40, 100, 255):
        q1 = a[30:90]
        q2 = a[10:50] + a[50 + min(W, 150) - 3:120 + min(W, 150)]
        out.append(group(f"wide{W}", a, [q1, q2, substitute(rng, q1, 4)], band=W))
    # a handful at 400
    a4 = rand_seq(rng, 420)
    qs = [a4[10:410], substitute(rng, a4[:400], 15), a4[5:200] + a4[203:405], a4[20:180] + "GATTACA" + a4[180:400]]
    out.append(group("long400", a4, qs))
    return out


def all_groups():
    return shape_groups() + band_groups() + tie_groups() + identity_boundary() + [random_set()]


def yardstick(g, **override):
    kw = dict(g["params"], **override)
    return [ref.align(q, g["anchor"], g["col"], g["width"], **kw) for q in g["queries"]]
