"""Inputs of the planted-edge tests of the k-mismatch scan (tests/test_kmm_edges.py).  A helper, not a test.

One database of 14 records (about 50 kb) on a seeded random ACGT background, with copies of the patterns written last at the places
where kmm_kernel changes behaviour: the 8192-start segment border and its overhang words, the 32-base word border of the packed
store, the last legal start of a record, a site cut by the end of a record, records shorter than a pattern, and copies with a counted
number of mismatches, a counted trailing match run, lower case, N, the other strand, a palindrome.

The patterns of lengths 4, 31, 32, 33, 63 and 64 are the SUFFIXES S_m of one 64-base string B.  So one copy of B ending at text
position e holds every S_m at start e - m (strand 0), and one copy of RC(B) at start s holds the reverse complement of every S_m at
start s (strand 1): a single plant puts all six lengths at one border, where six separate plants would overwrite one another.  Starts
8192 - m and 8192 - m + 1 are therefore planted on strand 0 and starts 8191 and 8192 on strand 1 (the kernel's table holds both
strands as entries of one kind); the records of 8255 and 8256 bases exist to hold RC(B) at 8191 and at 8192 to the last base.

Every plant is a tuple (category, record, start, pattern, strand) with the mismatch count and trailing match run it was built to
have; `database()` checks them against the final text (so no plant overwrote another), and `expected()` splits them by the rule of
include/mprime.h into the tuples a scan with (max_mm, term) must and must not report."""
import functools

import numpy as np

from multiprime_amd import iupac

SEG = 8192
LENGTHS = (4, 31, 32, 33, 63, 64)
RECORD_LENGTHS = (SEG + 40, 0, 65, SEG + 1, 33, 3, 31, 32, 63, 64, SEG - 1, SEG, SEG + 63, SEG + 64)
PREFIX = 5                                       # records of the "second load" prefix: two of them span the segment border
CATEGORIES = ("segment", "word", "last", "cut", "short", "mismatch", "term", "lower", "n", "strand", "palindrome")
NEVER_HIT = ("cut", "short")                     # categories without a legal site: nothing of theirs can be a must-hit
# (max_mm, term) of the full database; (3, m) runs on the equal-length sets, (64, 0) on a two-record cut
PARAMS = ((0, 0), (1, 4), (2, 0), (1, 70))
CUT = (3, 5)                                     # records [3, 5) = 8193 and 33 bases: the database of the (64, 0) case

_COMP = str.maketrans("ACGT", "TGCA")
_NEXT = str.maketrans("ACGT", "CGTA")            # a base that differs, for a planted mismatch


def rc(s):
    return s.translate(_COMP)[::-1]


def mutate(s, positions):
    s = list(s)
    for j in positions:
        s[j] = s[j].translate(_NEXT)
    return "".join(s)


def site(text, start, pat, strand):
    """(legal, mismatches, trailing match run) of `pat` at `start` of `text`, both strands compared in text orientation."""
    m, q = len(pat), pat if strand == 0 else rc(pat)
    if start < 0 or start + m > len(text):
        return False, None, None
    w = text[start:start + m].upper()
    mis = [j for j in range(m) if w[j] != q[j]]
    return True, len(mis), (m - 1 - mis[-1] if mis else m)


@functools.lru_cache(maxsize=None)
def database():
    """(records, patterns, plants): records as strings; patterns = {"S4": ..., ..., "S64": ..., "PAL": ...}; plants as dicts."""
    rng = np.random.default_rng(8192)

    def rnd(n):
        return "".join(rng.choice(list("ACGT"), size=n)) if n else ""
    B = rnd(64)
    if B[0] == B[63]:
        B = B[0].translate(_NEXT) + B[1:]
    half = rnd(16)
    pats = {f"S{m}": B[64 - m:] for m in LENGTHS}
    pats["PAL"] = half + rc(half)                # its own reverse complement: both strands hit at one start
    recs = [list(rnd(n)) for n in RECORD_LENGTHS]
    used = [np.zeros(n, bool) for n in RECORD_LENGTHS]
    plants = []

    def put(r, start, s):
        assert 0 <= start and start + len(s) <= len(recs[r]) and not used[r][start:start + len(s)].any(), (r, start, len(s))
        recs[r][start:start + len(s)] = s
        used[r][start:start + len(s)] = True

    def plant(cat, r, start, name, strand, mis=0, run=None, legal=True):
        plants.append(dict(cat=cat, r=r, start=start, pat=name, strand=strand, legal=legal, mis=mis,
                           run=len(pats[name]) if run is None else run))

    def put_B(cats, r, start):                   # every S_m on strand 0, ending where B ends
        put(r, start, B)
        for m in LENGTHS:
            for cat in cats:
                plant(cat, r, start + 64 - m, f"S{m}", 0)

    def put_rcB(cats, r, start, longest=64):     # every S_m on strand 1, starting where RC(B) starts
        put(r, start, rc(B)[:longest])
        for m in LENGTHS:
            if m <= longest:
                for cat in cats:
                    plant(cat, r, start, f"S{m}", 1)

    # segment border: 8192 - m (last site inside segment 0), 8192 - m + 1 (first into the overhang), 8191, 8192 (first of segment 1)
    put_B(("segment", "last"), 11, SEG - 64)                  # 8192 bases: the record ends with the segment
    put_B(("segment", "last"), 3, SEG - 63)                   # 8193 bases
    put_B(("segment",), 0, SEG - 64)                          # 8232 bases: the same site in a record that goes on
    put(0, SEG, pats["S32"])
    plant("segment", 0, SEG, "S32", 0)
    put_rcB(("segment",), 12, SEG - 1)                        # 8255 bases: RC(B) at 8191 to the last base
    plant("last", 12, SEG - 1, "S64", 1)
    put_rcB(("segment",), 13, SEG)                            # 8256 bases: RC(B) at 8192 to the last base
    plant("last", 13, SEG, "S64", 1)
    put(10, SEG - 1 - 64, rc(B))                              # 8191 bases: position 8191 is already past the end
    plant("last", 10, SEG - 1 - 64, "S64", 1)
    # word border of the packed store: starts 0, 31, 32, 33
    put_rcB(("word",), 0, 0)
    put_rcB(("word",), 10, 31)
    put_rcB(("word",), 11, 32)
    put_rcB(("word",), 3, 33)
    put_B(("word",), 12, 31)                                  # strand 0: S64 at 31, the shorter ones at 31 + 64 - m
    put_B(("word",), 13, 32)
    # record end: the last legal start in the short records
    put_B(("last",), 2, 1)                                    # 65 bases
    for r, m in ((4, 33), (6, 31), (7, 32)):                  # the record IS S_m: the shorter suffixes end with it
        put(r, 0, pats[f"S{m}"])
        for mm in LENGTHS:
            if mm <= m:
                plant("last", r, m - mm, f"S{mm}", 0)
    put(9, 64 - 33, pats["S33"])                              # 64 bases
    for mm in LENGTHS:
        if mm <= 33:
            plant("last", 9, 64 - mm, f"S{mm}", 0)
    # record end, cut site: the first m - 1 bases of every S_m end record 8 (63 bases), the last base opens record 9
    put(8, 0, B[:63])
    put(9, 0, B[63] + mutate(B[61:], range(3)))              # (and no chance copy of S4 behind it)
    for m in LENGTHS:
        plant("cut", 8, 64 - m, f"S{m}", 0, legal=False)
        plant("cut", 9, 0, f"S{m}", 0, mis=None)              # the other record: whatever stands there is no copy (counted from the text)
    # short records: the empty one, 3 bases, and every record shorter than the pattern
    put(5, 0, B[61:])
    for r, n in enumerate(RECORD_LENGTHS):
        for m in LENGTHS:
            if n < m:
                for strand in (0, 1):
                    plant("short", r, 0, f"S{m}", strand, legal=False)
    # counted copies, alternating between the free middles of records 0 and 3 (both in the prefix), at starts of every word phase
    cursor = {0: 130, 3: 131}
    turn = [0]

    def free(n):
        r = (0, 3)[turn[0] % 2]
        turn[0] += 1
        s = cursor[r]
        cursor[r] = s + n + 7
        assert cursor[r] < SEG - 100
        return r, s

    def put_copy(cat, name, text, strand=0, mis=0, run=None):
        r, s = free(len(text))
        put(r, s, text)
        plant(cat, r, s, name, strand, mis=mis, run=run)
        return r, s
    for m in LENGTHS:
        name, p = f"S{m}", pats[f"S{m}"]
        for k in (1, 2, 3, 4):                                # k mismatches in the first k columns: max_mm and max_mm + 1 for max_mm 0..3
            put_copy("mismatch", name, mutate(p, range(k)), mis=k, run=m - k)
        if m >= 5:
            put_copy("term", name, mutate(p, [m - 5]), mis=1, run=4)       # trailing run of exactly term = 4
        put_copy("term", name, mutate(p, [m - 4]), mis=1, run=3)           # and of term - 1
        put_copy("term", name, p)                                          # term = m: an exact copy has a run of exactly m,
        put_copy("term", name, mutate(p, [0]), mis=1, run=m - 1)           # a mismatch in the first column leaves m - 1
        put_copy("lower", name, p.lower())
        put_copy("n", name, p[:1] + "N" + p[2:], mis=1, run=m - 2)         # an N inside: one mismatch
        put_copy("n", name, p[:m - 2] + "N" + p[m - 1:], mis=1, run=1)     # an N in the last columns: the term rejects it
        put_copy("strand", name, rc(p), strand=1)
    for text, mis, run in ((pats["PAL"], 0, 32), (mutate(pats["PAL"], [3]), 1, 28), (pats["PAL"].lower(), 0, 32)):
        r, s = put_copy("palindrome", "PAL", text, 0, mis, run)
        plant("palindrome", r, s, "PAL", 1, mis=mis, run=run)              # the text equals RC(PAL) as well: same columns differ
    put(10, 4090, pats["PAL"])                                             # and one across a word border of a one-segment record
    plant("palindrome", 10, 4090, "PAL", 0)
    plant("palindrome", 10, 4090, "PAL", 1)

    seqs = ["".join(r) for r in recs]
    for p in plants:                                          # what was planted is what stands in the text
        legal, mis, run = site(seqs[p["r"]], p["start"], pats[p["pat"]], p["strand"])
        assert legal == p["legal"], p
        if legal and p["mis"] is None:
            p["mis"], p["run"] = mis, run
        assert not legal or (mis, run) == (p["mis"], p["run"]), (p, mis, run)
    return tuple(seqs), pats, tuple(plants)


def pattern_set(name):
    """Names of a pattern set: "one" (at most 32 bases: the one-word kernel), "two" (one longer pattern puts all of them on the
    two-word kernel), "eq<m>" (equal lengths, for term = m)."""
    if name == "one":
        return ["S4", "S31", "S32", "PAL"]
    if name == "two":
        return [f"S{m}" for m in LENGTHS] + ["PAL"]
    m = int(name[2:])
    return [f"S{m}"] + (["PAL"] if m == 32 else [])


def encode(seqs):
    data = np.frombuffer("".join(seqs).encode(), np.uint8)
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return data, off


def encode_patterns(strings):
    codes = iupac.MASK_LUT[np.frombuffer("".join(strings).encode(), np.uint8)]
    poff = np.zeros(len(strings) + 1, np.int32)
    np.cumsum([len(p) for p in strings], out=poff[1:])
    return codes, poff


def expected(names, max_mm, term, rows=None):
    """(must_hit, must_not_hit, by_category) for a scan of records `rows` = (first, end) with the pattern set `names`: sets of
    (record, start, pattern index, strand), records counted from `first`; by_category[cat] = [n must-hit, n must-not-hit]."""
    _, pats, plants = database()
    first, end = rows or (0, len(RECORD_LENGTHS))
    hit, miss, by = set(), set(), {c: [0, 0] for c in CATEGORIES}
    for p in plants:
        if p["pat"] not in names or not first <= p["r"] < end:
            continue
        t = (p["r"] - first, p["start"], names.index(p["pat"]), p["strand"])
        ok = p["legal"] and p["mis"] <= max_mm and p["run"] >= term
        (hit if ok else miss).add(t)
        by[p["cat"]][0 if ok else 1] += 1
    assert not hit & miss
    return hit, miss, by
