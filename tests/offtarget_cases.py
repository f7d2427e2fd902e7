"""Inputs of the planted-edge tests of the off-target screen (tests/test_offtarget_edges.py).  A helper, not a test.

Every case is a store, reads with primer ids and mismatch budgets, `term` and a size range; everything is seeded or written out.
What a case contains is asserted by the test on the model of tests/offtarget_ref.py, never taken from here.

a  the planted database of tests/kmm_cases.py (14 records, 49610 bases), the reads of its "two" set in the order S64 .. S4 so that the
   long reads have the small indices, two reads per primer id; three parameter sets and the first of them with the reads reversed.
b  records kmm_cases.CUT (8193 and 33 bases), every read in ascending length with a budget that admits every legal start: a full map.
c  stores of 8191, 8192 and 8193 bases of 'A' with runs of C (forward sites of the reads CCCC and CCCCC) and runs of G (their reverse
   sites) at chosen store offsets, empty records first, last and between, one record shorter than every read.
d  255, 256 and 257 records of 0 to 40 random bases, a quarter of them empty, two 6-base reads planted in a third of them."""
import functools
from collections import namedtuple

import numpy as np

import kmm_cases as kc
from offtarget_ref import rc

Case = namedtuple("Case", "name seqs reads primer budgets term lo hi")

A_ORDER = ("S64", "S63", "S33", "S32", "S31", "PAL", "S4")
A_PARAMS = {"a1": ((3, 3, 2, 2, 2, 1, 0), 0, 20, 9000),          # four launches; every suffix of B on one start of strand 1
            "a2": ((2, 2, 1, 1, 1, 1, 1), 4, 30, 400),           # dead starts
            "a3": ((3, 3, 2, 2, 2, 1, 1), 0, 8000, 8300)}        # whole-row rejects
A_CLASSES = (0, 1, 0, 1, 0, 1, 1)


def case_a(name):
    seqs, pats, _ = kc.database()
    budgets, term, lo, hi = A_PARAMS[name[:2]]
    reads = [pats[n] for n in A_ORDER]
    if name.endswith("rev"):
        reads, budgets = reads[::-1], budgets[::-1]
    return Case(name, list(seqs), reads, [100 + i // 2 for i in range(len(reads))], list(budgets), term, lo, hi)


def case_b():
    seqs, pats, _ = kc.database()
    reads = sorted((pats[n] for n in kc.pattern_set("two")), key=len)
    return Case("b", list(seqs[kc.CUT[0]:kc.CUT[1]]), reads, [200 + i for i in range(len(reads))], [64] * len(reads), 0, 100, 110)


# ---- c: sparse sites on the borders of the map's chunks ---------------------------------------------------------------------------------
C_READS = ("CCCC", "CCCCC")
C_PRIMER = (7, 9)
C_STEP = 30                                      # a reverse site this far behind its forward site: a product of 31 bases
C_LAYOUT = (0, 300, 0, 4700, 3, 0, None, 0)      # record lengths; None: what is left of the total
C_INNER = 3                                      # the inner record whose first and last legal start are planted (store offsets 300, 4996)


def case_c(total, lo=20, hi=40):
    """(case, forward, reverse): the store offsets of the planted sites by strand, as sets — what the model must find, no more."""
    lengths = [total - sum(n for n in C_LAYOUT if n is not None) if n is None else n for n in C_LAYOUT]
    off = np.concatenate([[0], np.cumsum(lengths)])
    text = ["A"] * total
    last = total - 4                             # the last legal start of the store
    inner_first, inner_last = int(off[C_INNER]), int(off[C_INNER + 1]) - 4
    c_runs = [(0, 4), (63, 5), (255, 5), (266, 4), (inner_first, 4), (4095, 5), (inner_last, 4), (6000, 4), (last, 4)]
    # the partner of inner_last lies in a later record (a join on bare store offsets would pair them); `last` has none; 296 is the last
    # legal start of record 1, a reverse site, and touches the forward site at the first base of record 3
    g_runs = [(o + C_STEP, n) for o, n in c_runs if o != last]
    forward, reverse = set(), set()
    for runs, letter, found in ((c_runs, "C", forward), (g_runs, "G", reverse)):
        for o, n in runs:
            assert text[o:o + n] == ["A"] * n, (o, n)
            text[o:o + n] = letter * n
            found.update(range(o, o + n - 3))
    text[int(off[4]):int(off[5])] = "CCC"        # the short record: C to the right of inner_last's CCCC, and no site of its own
    text = "".join(text)
    seqs = [text[off[i]:off[i + 1]] for i in range(len(lengths))]
    return Case(f"c{total}" + ("" if (lo, hi) == (20, 40) else "none"), seqs, list(C_READS), list(C_PRIMER), [0, 0], 0, lo, hi), forward, reverse


def c_required(total):
    """The forward map indices the case is built for."""
    return {0, 63, 64, 255, 256, 4095, 4096, total - 4, 300, 4996}


# ---- d: many short records --------------------------------------------------------------------------------------------------------------
D_READS = ("ACGGTC", "TTGCAG")
D_PRIMER = (11, 5)


def case_d(n):
    rng = np.random.default_rng(n)
    seqs = []
    for i in range(n):
        planted = (n - 1 - i) % 3 == 0           # the last record always
        if not planted and i % 8 in (2, 5, 7):
            seqs.append("")
            continue
        if not planted:
            seqs.append("".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 41)))))
            continue
        s = list(rng.choice(list("ACGT"), size=int(rng.integers(24, 41))))
        f, r = D_READS if (i // 3) % 2 == 0 else D_READS[::-1]     # every other planted record the other way round: its first forward read is 1
        start = int(rng.integers(0, 3))
        stop = int(rng.integers(start + 12, len(s) - 5))           # length stop - start + 1 in 13 .. 35
        s[start:start + 6] = f
        s[stop:stop + 6] = rc(r)
        seqs.append("".join(s))
    return Case(f"d{n}", seqs, list(D_READS), list(D_PRIMER), [1, 0], 0, 10, 30)


NAMES = ("a1", "a2", "a3", "a1rev", "b", "c8191", "c8192", "c8193", "c8192none", "d255", "d256", "d257")


@functools.lru_cache(maxsize=None)
def get(name):
    if name.startswith("a"):
        return case_a(name)
    if name == "b":
        return case_b()
    if name.startswith("c"):
        return case_c(int(name[1:5]), *((50, 60) if name.endswith("none") else ()))[0]
    return case_d(int(name[1:]))
