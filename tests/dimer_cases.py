"""Seeded case builders for tests/test_dimer_edges.py: primers for mp_dimer_scan / mp_dimer_pairs placed on the edges of the kernels in
multiprime_amd/csrc/dimer.hip.  Every builder returns the primers plus what the case is meant to contain; the test asserts that content
from tests/dimer_ref.py before anything runs on a GPU."""
import random
from functools import lru_cache
from itertools import product

import dimer_ref as R

LENGTHS = [1, 2, 3, 4, 5, 6, 17, 18, 19, 21, 22, 31, 32]
LONG_LENGTHS = [33, 48, 63, 64]


def plain(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def holding(rng, site, length, d2):
    """A plain partner of `length` bases that holds `site` d2 bases before its 3' end."""
    left = length - len(site) - d2
    assert left >= 0
    return plain(rng, left) + site + plain(rng, d2)


# ---- end lengths, plane widths, table corners -------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def length_ladder(long):
    """The primers.  For each length an x; partners of its own length, of 32 and (long) of 64 bases carry RC of its longest
    mode-0 end (and a second set RC of x[1:], mode 1's longest) flush, one base before the 3' end and at the partner's first base;
    partners shorter than the end; an 18-base palindrome and three copies of one primer.  The long x are GC-rich (an end with >= 32 G/C)."""
    rng = random.Random(20240 + long)
    seqs, xs = [], []
    for lx in LENGTHS + (LONG_LENGTHS if long else []):
        x = plain(rng, lx, "GCGCGCAT" if lx >= 48 else "ACGT")
        xs.append(len(seqs))
        seqs.append(x)
        for end in (x[-min(18, lx):], x[1:]):
            if not end:
                continue
            site = R.rc(end)
            for ly in sorted({lx, 32, 64} if long else {lx, 32}):
                for d2 in sorted({0, 1, ly - len(site)}):
                    if 0 <= d2 <= ly - len(site):
                        seqs.append(holding(rng, site, ly, d2))
            if len(site) >= 2:                                        # shorter than the end: holds RC of a shorter end, flush at both sides
                seqs.append(site[:len(site) - 1])
                seqs.append(site[:max(1, len(site) // 2)])
    half = plain(rng, 9)
    seqs.append(half + R.rc(half))                                    # pairs with itself over its whole length
    seqs += [seqs[xs[7]]] * 3                                         # duplicates of the 18-mer
    return list(dict.fromkeys(seqs[:-3])) + seqs[-3:]


# ---- deltaG on its rounding boundary ---------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def boundary_ends(per_class=2):
    """{(rounded deltaG, class): [ends]} for -5.01, -5.0, -4.99 and the classes plain / ta (ends in TA) / sym (self-pairing halves), from an
    enumeration of every concrete end of 5..8 bases and of the 9-base ends in TA (no shorter end in TA rounds to -5.0 or -4.99); only
    ends none of whose shorter suffixes (>= 5) is below -5, so the full end alone decides.  The first and the last `per_class` found of
    each are kept.  No symmetric end of 5..9 bases rounds to -5.01 or -4.99."""
    found = {}
    for n in range(5, 10):
        for t in product("ACGT", repeat=n if n < 9 else 7):
            e = "".join(t) + ("" if n < 9 else "TA")
            g = R.delta_g(e)
            if g in (-5.01, -5.0, -4.99) and all(R.delta_g(e[-k:]) >= -5 for k in range(5, n)):
                cls = "sym" if R.symmetric(e) else "ta" if e.endswith("TA") else "plain"
                found.setdefault((g, cls), []).append(e)
    return {k: list(dict.fromkeys(v[:per_class] + v[-per_class:])) for k, v in found.items()}


@lru_cache(maxsize=None)
def boundary_set():
    """(primers, [(rounded deltaG, class, x, flush partner, partner one base off)]): each end is the 3' end of a 20-base x whose 5' part
    pairs with nothing planted; one partner holds RC(end) at its 3' end, one a base before it."""
    rng = random.Random(501)
    seqs, plan = [], []
    for (g, cls), ends in sorted(boundary_ends().items()):
        for e in ends:
            while True:
                x = plain(rng, 20 - len(e)) + e
                flush = plain(rng, 22 - len(e)) + R.rc(e)
                off = plain(rng, 21 - len(e)) + R.rc(e) + rng.choice([b for b in "ACGT" if b != R.rc(x[-len(e) - 1])])
                # nothing but the planted end may match: a longer end, or a second site, would decide instead
                if all(len(R.matches(x, y, m)) == len(e) - 4 and R.matches(x, y, m)[0][0] == len(e) for y in (flush, off) for m in (0, 1)):
                    break
            plan.append((g, cls, len(seqs), len(seqs) + 1, len(seqs) + 2))
            seqs += [x, flush, off]
    return seqs, plan


# ---- degenerate primers ----------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def degenerate_light():
    """(primers, named index pairs).  2-, 3- and 4-member codes in ends and partners (at most 48 expansions per primer, so every ordered
    pair can be walked); `first`: both expansions of x's 12-base end occur in y, the second one earlier in y — expansion 0 is reported."""
    rng = random.Random(77)
    e0, e1 = "GATTCCAGGTCA", "GATTCCGGGTCA"                             # the end GATTCCRGGTCA
    x_first, y_first = "GATTCCRGGTCA", R.rc(e1) + R.rc(e0)
    body = plain(rng, 6)
    xa = body + "ACRTGGHCATNGTCCATG"                                    # 2 x 3 x 4 = 24 expansions of its 18-base end
    ya = plain(rng, 4) + R.rc(R.expand(xa[-18:])[17])                   # a plain partner: one expansion of the end, flush
    yb = plain(rng, 3) + R.rc("ACRTGGHCATAGTCCATG") + "W"               # a degenerate partner one base off (12 expansions)
    xc = plain(rng, 9) + "SGWTCCAYK"
    yc = R.rc(xc[-9:]).replace("S", "G", 1) + plain(rng, 8)             # RC of the short end at the partner's first base
    seqs = [x_first, y_first, xa, ya, yb, xc, yc]
    for _ in range(9):
        s = list(plain(rng, rng.randint(6, 30)))
        for p in rng.sample(range(len(s)), 2):
            s[p] = rng.choice("RYMKSWHBVDN")
        seqs.append("".join(s))
    return seqs, {"first": (0, 1), "plain_partner": (2, 3), "degenerate_partner": (2, 4)}


@lru_cache(maxsize=None)
def degenerate_heavy():
    """(primers, n_new, named index pairs): walked in mode 1 with n_new = 2 and as the pair list of the same pairs, never all against all
    (the heavy primers against themselves would be 10^7 combinations on the CPU).
    `last_end`: x has six N in its 18-base end (4096 expansions, 19 bases so both modes try that end) and only the last one, every N
    = C, occurs in y.  `late_y`: y starts with eight 3-member codes and an N (26 244 expansions); RC of the 9-base x occurs only in the
    last of them, at y's first base, so far from the 3' end that only a threshold below every Loss reports it."""
    x_last = "G" + "NNNNNN" + "TGACTTGCAATG"
    y_last = "TTGACCA" + R.rc("CCCCCC" + "TGACTTGCAATG")
    y_late = "HBVDHBVDN" + "TTGGTTGGTTGGTTGGTTGG"
    x_late = R.rc("".join(R.MEMBERS[c][-1] for c in y_late[:9]))
    seqs = [y_last, x_late, y_late, x_last]
    return seqs, 2, {"last_end": (3, 0), "late_y": (1, 2)}


# ---- queue and hit buffer of dimer_rows_kernel -----------------------------------------------------------------------------------------
STRIDE = 256


def drain_set(strides, long=False, seed=9):
    """(primers, [(hitters, passers)] per stride as built).  Primer 0 is the row under test; `strides` gives, per 256 partners from y = 0,
    how many hold RC of its 18-base end flush (hitters) and how many pass the bit-plane filter without any hit at 3.96 (passers); the
    rest of a stride, except in the last one, are fillers that fail the filter.  y = 0 is primer 0 itself: it is a passer of its own
    row when the first stride has passers, else a filler.  long: one 33-base primer that pairs with nothing is appended."""
    rng = random.Random(seed)
    self_passes = strides[0][1] > 0
    while True:
        end = plain(rng, 18)
        x = (R.rc(end[-5:]) + plain(rng, 4) if self_passes else plain(rng, 6)) + end
        if R.passes_filter(x, x, 5) == self_passes and R.pair_hit(x, x, 0, 3.0) is None and R.pair_hit(x, x, 1, 3.0) is None \
                and not R.passes_filter(R.rc(end), R.rc(end), 5):         # the hitters' common 3' end does not pair with itself
            break

    def kind(y):
        if not R.passes_filter(x, y, 5):
            return "filler"
        return "hitter" if R.pair_hit(x, y, 0, 3.96) else "passer"

    def make(want):
        while True:
            if want == "hitter":
                y = plain(rng, rng.randint(0, 6)) + R.rc(end)
            elif want == "passer":                                    # RC of the last five bases, far from the 3' end, the sixth differing
                y = plain(rng, rng.randint(0, 3)) + R.rc(end[-5:]) + rng.choice([b for b in "ACGT" if b != R.rc(end[-6])]) + plain(rng, 12)
            else:
                y = plain(rng, rng.randint(18, 24))
            if kind(y) == want and (R.pair_hit(x, y, 1, 3.0) is not None) == (want == "hitter"):      # the same in get_Maxprimerset's mode
                return y

    seqs = [x]
    for i, (n_hit, n_pass) in enumerate(strides):
        own = 1 if i == 0 and self_passes else 0
        part = [make("hitter") for _ in range(n_hit)] + [make("passer") for _ in range(n_pass - own)]
        room = STRIDE - (1 if i == 0 else 0) - len(part)
        assert room >= 0
        if i + 1 < len(strides):
            part += [make("filler") for _ in range(room)]
        rng.shuffle(part)
        seqs += part
    if long:
        while True:
            y = plain(rng, 33)
            if not any(R.passes_filter(a, b, 5) for a, b in ((x, y), (y, x), (y, y))):
                break
        seqs.append(y)
    return seqs


def drain_counts(seqs):
    """Per stride of 256 partners of primer 0 (mode 0: y = 0 ..): (hitters, passers) as the model sees them."""
    x, out = seqs[0], []
    for y0 in range(0, len(seqs), STRIDE):
        kinds = [(R.passes_filter(x, y, 5), R.pair_hit(x, y, 0, 3.96) is not None) for y in seqs[y0:y0 + STRIDE]]
        out.append((sum(1 for f, h in kinds if h), sum(1 for f, h in kinds if f and not h)))
        assert all(f for f, h in kinds if h)
    return out


def full(n):
    return (min(n, STRIDE), 0)


def hit_row(n_hits):
    """Strides of a row with exactly n_hits hitters packed from y = 1 (255 beside primer 0, which passes its own filter, then 256 each)."""
    strides, left = [(min(255, n_hits), 1)], n_hits - min(255, n_hits)
    while left > 0:
        strides.append(full(left))
        left -= min(left, STRIDE)
    return strides


DRAINS = {
    # filter survivors per stride
    "q255_1": [(100, 155), (1, 0)],                 # 255 wait after the first stride, the 256th arrives in the second
    "q256": [(100, 156)],                           # exactly one queue load in the only stride
    "q511": [(100, 155), (200, 56)],                # 255 wait, 256 arrive: the fullest queue there can be
    "late300": [(0, 0), (0, 0), (200, 56), (30, 14)],
    # hits per row
    "h512": hit_row(512), "h513": hit_row(513), "h1023": hit_row(1023), "h1024": hit_row(1024), "h1025": hit_row(1025),
    # 512 records held and not flushed (255 + 256 + 1), then a drain of 511: 1023 records in the 1024-record buffer
    "held512_then_511": [(255, 1), (256, 0), (1, 255), (255, 0), (256, 0)],
    "passers600": [(0, 256), (0, 256), (0, 88)],    # the queue drains twice and on the last stride, nothing is ever held
}


# ---- host selection ---------------------------------------------------------------------------------------------------------------------
def random_primers(seed, n):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        s = list(plain(rng, rng.randint(18, 24)))
        if rng.random() < 0.3:
            s[rng.randrange(len(s))] = rng.choice("RYMKSW")
        out.append("".join(s))
    for _ in range(n // 3):                                           # planted 3' complementarity
        i, j = rng.randrange(n), rng.randrange(n)
        site = R.rc(R.expand(out[i][-rng.randint(6, 12):])[0])
        pos = len(out[j]) - len(site) - rng.randint(0, 2)
        out[j] = out[j][:pos] + site + out[j][pos + len(site):]
    return out


SCAN_SIZES = {255: (32767, 64), 256: (33024, 16), 723: (262087, 16), 724: (262812, 1)}          # n: (mode-0 pairs visited, lanes per pair)
LIST_SIZES = {32768: 64, 32769: 16, 262144: 16, 262145: 1}                                       # pairs in the list: lanes per pair


def pair_list(seed, n_primers, n_pairs):
    rng = random.Random(seed)
    return [(rng.randrange(n_primers), rng.randrange(n_primers)) for _ in range(n_pairs)]
