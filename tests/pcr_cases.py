"""Inputs of the planted-edge tests of the exact in-silico PCR scan (tests/test_pcr_edges.py).  A helper, not a test.

`model()` is the operation the reference script's way (extract_PCR_product_V1.py:189-216) on `str`: re.search, str.split,
Product = sequence + line[1], expansions in iupac.expand's order.  It shares no code with the checker (oracle/mprime_oracle.c).
`occurrences()` counts what the block kernel's occurrence list counts.

`calls()` returns every call of every group.  A group fixes the per-call properties of pcr_scan_device (one or two pattern words,
prefix filter on or off) through the primer lengths of its calls:

    G_short  4, 5, 7            filter off by itself, one word
    G_8      8                  the shortest length the filter admits
    G_word   12, 20, 31, 32     one word, the k == 32 mask
    G_two    12, 33, 63, 64     two words with short primers among them
    G_64     64                 two words only
    G_table  20 and 40          pattern tables of exactly 4096 entries (block kernel) and of 4097 (the whole call rolls)

A call is (name, records, primer pairs) plus what the planted situations must give: `expect` = (situation, pair, record, tuple) and
`counts` = (record, occurrences).  Records are seeded random A/C/G/T with the sites written on top; every chance copy of a pattern of
the call that touches a background base is then broken by changing such a base, so that no site stands outside the planted spans
(`unplanted()` checks that with str.find)."""
import functools
import re

import numpy as np

from multiprime_amd import iupac

SEG = 4096                                       # kPcrSeg: positions per LDS segment
HITS = 3072                                      # kPcrHits: the occurrence list
TABLE = 4096                                     # patterns per call of the block kernel
NONE = (-1, -1, -1, -1)
GAP = 30                                         # background bases between planted sites
BORDER_GAP = 40                                  # the reverse site of a border record starts this far behind the forward site
# primer lengths (forward, reverse) of the pairs of a group's main call; "selfov_in": the pair whose RC(R) lies inside F itself
GROUPS = {
    "G_short": dict(main=(7, 5), selfov=(4, 7), selfov_in=(7, 4), pal=4, dege=(5, 4), extras=[(5, 7)]),
    "G_8": dict(main=(8, 8), selfov=(8, 8), selfov_in=None, pal=8, dege=(8, 8), extras=[]),
    "G_word": dict(main=(32, 20), selfov=(20, 31), selfov_in=(31, 12), pal=32, dege=(31, 32), extras=[(12, 32)]),
    "G_two": dict(main=(64, 12), selfov=(12, 63), selfov_in=(33, 12), pal=12, dege=(33, 63), extras=[(63, 33)]),
    "G_64": dict(main=(64, 64), selfov=(64, 64), selfov_in=None, pal=64, dege=(64, 64), extras=[]),
}
OCC_GROUPS = {"G_8": (8, 8), "G_two": (33, 12)}  # occurrence-list calls: one pair each, these lengths
OCC_COUNTS = (HITS - 1, HITS, HITS + 1, 6000)    # last two list-served counts, the first fall-back, about twice the list
GROUP_NAMES = tuple(GROUPS) + ("G_table",)
FILTERED = ("G_8", "G_word", "G_two", "G_64", "G_table")       # groups whose shortest primer has >= 8 bases: prefix filter on
# what one GPU test runs: the calls of a group, or one call of G_table (its rolling calls are the slowest of all)
UNITS = tuple((g, None) for g in GROUPS) + tuple(("G_table", i) for i in range(6))
UNIT_IDS = tuple(g if i is None else "%s-%d" % (g, i) for g, i in UNITS)


def unit_calls(unit):
    group, i = unit
    return calls(group) if i is None else calls(group)[i:i + 1]


# ---- the reference's expression ------------------------------------------------------------------------------------------------
def model(seqs, primers):
    """[pair][record] = (fi, p1, ri, q) of the first forward expansion that occurs and whose Product holds RC(a reverse expansion);
    (-1, -1, -1, -1) where none does."""
    seqs = tuple(seqs)
    return [list(_model_pair(F, R, seqs)) for F, R in primers]


@functools.lru_cache(maxsize=256)
def _model_pair(F, R, seqs):
    """One pair on every record (a pair is decided by itself: calls that share records and a pair share its rows)."""
    rows = []
    for s in seqs:
        res = NONE
        for fi, f in enumerate(iupac.expand(F)):
            m = re.search(f, s)
            if not m:
                continue
            parts = s.split(f)
            product = f + parts[1]
            for ri, r in enumerate(iupac.expand(R)):
                m2 = re.search(iupac.revcomp(r), product)
                if m2:
                    res = (fi, m.start(), ri, m.start() + m2.start())
                    break
            if res != NONE:
                break
        rows.append(res)
    return tuple(rows)


def patterns_of(primers):
    """The pattern table of a call: per pair every forward expansion, then RC(every reverse expansion)."""
    pats = []
    for F, R in primers:
        pats += iupac.expand(F)
        pats += [iupac.revcomp(r) for r in iupac.expand(R)]
    return pats


def _starts(seq, pat):
    i = seq.find(pat)
    while i >= 0:
        yield i
        i = seq.find(pat, i + 1)


def occurrences(seq, patterns):
    """Entries of the block kernel's occurrence list for one record: start positions, overlapping ones included, at which a pattern
    matches entirely inside the record, summed over the table's entries (the number of distinct starts when no entry equals or
    begins another, as in the occurrence-list calls)."""
    return sum(1 for p in patterns for _ in _starts(seq, p))


# ---- builders ------------------------------------------------------------------------------------------------------------------
class Call:
    def __init__(self, group, name, pairs):
        self.group, self.name = group, name
        self.pair_names = list(pairs)
        self.primers = [pairs[n] for n in self.pair_names]
        self.records, self.planted = [], []      # planted[r]: bool per base, True inside a planted span
        self.expect, self.counts = [], []

    def pair(self, name):
        return self.pair_names.index(name)

    def sub(self, name, pair_names):
        """The same records with some of the pairs (a call of its own)."""
        c = Call(self.group, name, {n: self.primers[self.pair(n)] for n in pair_names})
        c.records, c.planted = self.records, self.planted
        c.expect = [e for e in self.expect if e[1] in pair_names]
        return c


class _Builder:
    def __init__(self, call, rng):
        self.c, self.rng = call, rng
        cls = lambda s: "".join("[" + iupac.MEMBERS[ch] + "]" for ch in s)       # noqa: E731
        sides = {(F, False) for F, _ in call.primers} | {(R, True) for _, R in call.primers}
        self.rx = [(re.compile("(?=" + cls(iupac.revcomp(p) if rc else p) + ")"), len(p)) for p, rc in sorted(sides)]

    def rnd(self, n):
        return "".join(self.rng.choice(list("ACGT"), size=n)) if n else ""

    def rec(self, n, plants=()):
        chars, prot = list(self.rnd(n)), np.zeros(n, bool)
        for start, text in plants:
            assert 0 <= start and start + len(text) <= n and not prot[start:start + len(text)].any(), (self.c.name, n, start, len(text))
            chars[start:start + len(text)] = text
            prot[start:start + len(text)] = True
        for _ in range(10000):                   # break every chance copy that touches the background
            s, clean = "".join(chars), True
            for rx, L in self.rx:
                for m in rx.finditer(s):
                    free = [j for j in range(m.start(), m.start() + L) if not prot[j]]
                    if free:
                        j = free[int(self.rng.integers(len(free)))]
                        chars[j] = "ACGT"[("ACGT".index(chars[j]) + 1 + int(self.rng.integers(3))) % 4]
                        clean = False
            if clean:
                break
        else:
            raise AssertionError("background of %s does not come clean" % self.c.name)
        self.c.records.append("".join(chars))
        self.c.planted.append(prot)
        return len(self.c.records) - 1

    def want(self, situation, pair, r, res):
        self.c.expect.append((situation, pair, r, tuple(res)))
        if pair == "main" and "main_dup" in self.c.pair_names:                   # (i) the same pair listed twice
            self.c.expect.append((situation + "/listed twice", "main_dup", r, tuple(res)))


def _borderless(s):
    return all(s[:k] != s[-k:] for k in range(1, len(s)))


def _plain(rng, n, avoid=(), first=None):
    """A random concrete primer that does not overlap itself, holds none of `avoid` and lies in none of them, both strands."""
    for _ in range(100000):
        s = "".join(rng.choice(list("ACGT"), size=n))
        if first:
            s = first + s[1:]
        both = (s, iupac.revcomp(s))
        if _borderless(s) and not any(a in b or b in a for a in avoid for b in both) and (n < 4 or "ACA" not in s and "TGT" not in s):
            return s
    raise AssertionError("no primer of %d bases" % n)


def _run(n):
    return ("AC" * (n // 2 + 1))[:n]


def _main_pairs(rng, spec):
    lf, lr = spec["main"]
    F = _plain(rng, lf)
    R = _plain(rng, lr, [F], first=iupac.revcomp(F[0]))          # RC(R) ends with F's first base: (b) lets the two sites share it
    used = [F, R]
    pairs = {"main": (F, R)}
    lf, lr = spec["selfov"]
    pairs["selfov"] = (_run(lf), _plain(rng, lr, used))
    used.append(pairs["selfov"][1])
    if spec["selfov_in"]:
        lf, lr = spec["selfov_in"]
        pairs["selfov_in"] = (_run(lf), iupac.revcomp(_run(lf)[1:1 + lr]))
    for _ in range(100000):
        half = "".join(rng.choice(list("ACGT"), size=spec["pal"] // 2))
        P = half + iupac.revcomp(half)
        if _borderless(P) and not any(P in u or u in P for u in used) and "ACA" not in P and "TGT" not in P:
            break
    pairs["pal"] = (P, P)
    used.append(P)
    lf, lr = spec["dege"]
    f, r = _plain(rng, lf, used), None
    a, b = lf // 3, 2 * lf // 3
    Fd = f[:a] + "R" + f[a + 1:b] + "Y" + f[b + 1:]              # expansions in order: (A,C) (A,T) (G,C) (G,T)
    used += iupac.expand(Fd)
    r = _plain(rng, lr, used)
    Rd = r[:lr // 2] + "R" + r[lr // 2 + 1:]
    used += iupac.expand(Rd)
    pairs["dege"] = (Fd, Rd)
    pairs["j"] = (iupac.revcomp(R), iupac.revcomp(F))           # (j) F = RC(R of main), RC(R) = F of main: duplicate table entries
    for i, (lf, lr) in enumerate(spec["extras"]):
        f = _plain(rng, lf, used)
        used.append(f)
        r = _plain(rng, lr, used)
        used.append(r)
        pairs["extra%d" % i] = (f, r)
    pairs["main_dup"] = pairs["main"]
    return pairs


def _mutants(site):
    """The site with one base lower-cased, one replaced by N, one by the IUPAC letter R."""
    j = len(site) // 2
    return (("lower", site[:j] + site[j].lower() + site[j + 1:]), ("N", site[:j] + "N" + site[j + 1:]), ("R", site[:j] + "R" + site[j + 1:]))


def _main_call(group, spec, rng):
    c = Call(group, group + "/main", _main_pairs(rng, spec))
    b = _Builder(c, rng)
    f, R = c.primers[c.pair("main")]
    rr = iupac.revcomp(R)
    L, lr = len(f), len(rr)
    assert rr[-1] == f[0] and L == max(len(p) for pr in c.primers for p in pr)
    b.want("empty record first", "main", b.rec(0), NONE)
    # 1. borders
    for border in (SEG, 2 * SEG):
        for s in (range(SEG - L, SEG + 1) if border == SEG else (border - L, border - 1, border)):
            r = b.rec(s + L + BORDER_GAP + lr + 7, [(s, f), (s + L + BORDER_GAP, rr)])
            b.want("forward site at %d" % s, "main", r, (0, s, 0, s + L + BORDER_GAP))
    for q in sorted({SEG - lr + 1, SEG - lr // 2, SEG - 1}):
        r = b.rec(q + lr + 50, [(q - 60 - L, f), (q, rr)])
        b.want("reverse site straddles %d from %d" % (SEG, q), "main", r, (0, q - 60 - L, 0, q))
    for n in (SEG - 1, SEG, SEG + 1):
        r = b.rec(n, [(n - lr - 50 - L, f), (n - lr, rr)])
        b.want("reverse site ends a record of %d" % n, "main", r, (0, n - lr - 50 - L, 0, n - lr))
    b.want("empty record in the middle", "main", b.rec(0), NONE)
    # 2. record ends
    b.want("forward site at the last legal start", "main", b.rec(300, [(300 - L, f)]), NONE)
    h = L // 2
    b.want("record ends with half of F", "main", b.rec(200, [(200 - h, f[:h])]), NONE)
    b.want("record begins with the other half of F", "main", b.rec(200, [(0, f[h:]), (L - h + BORDER_GAP, rr)]), NONE)
    P = c.primers[c.pair("pal")][0]
    h = len(P) // 2
    b.want("record ends with half of a palindromic F", "pal", b.rec(150, [(150 - h, P[:h])]), NONE)
    b.want("record begins with the other half of a palindromic F", "pal", b.rec(150, [(0, P[h:])]), NONE)
    h = lr // 2
    b.want("record ends with half of RC(R)", "main", b.rec(200, [(50, f), (200 - h, rr[:h])]), NONE)
    b.want("record begins with the other half of RC(R)", "main", b.rec(150, [(0, rr[h:])]), NONE)
    b.want("record one base shorter than F", "main", b.rec(L - 1, [(0, f[:-1])]), NONE)
    b.want("one-base record", "main", b.rec(1), NONE)
    # 3. the rule
    x = 50 + L + GAP
    r = b.rec(400, [(50, f), (x, f), (x + L + GAP, rr)])
    b.want("(a) RC(R) only behind the second F", "main", r, NONE)
    r = b.rec(400, [(50, f + f), (50 + 2 * L + GAP, rr)])
    b.want("(a) second F directly behind the first", "main", r, NONE)
    r = b.rec(400, [(50, f), (x, rr + f)])
    b.want("(b) RC(R) ends at the second F", "main", r, (0, 50, 0, x))
    r = b.rec(400, [(50, f), (x, rr[:-1] + f)])
    b.want("(b) RC(R) ends one base into the second F", "main", r, NONE)
    so, Rso = c.primers[c.pair("selfov")]
    lf, rso = len(so), iupac.revcomp(Rso)
    q = 50 + lf + 2 + 10
    r = b.rec(500, [(50, _run(lf + 2)), (q, rso), (q + len(rso) + GAP, so)])
    b.want("(c) overlapping copy of F two bases on is no split point", "selfov", r, (0, 50, 0, q))
    n_run = 3 * lf + 1
    r = b.rec(600, [(50, _run(n_run)), (50 + n_run + 10, rso)])
    b.want("(c) run of the repeat unit: Product ends at the next non-overlapping copy", "selfov", r, NONE)
    if "selfov_in" in c.pair_names:
        lf_in = len(c.primers[c.pair("selfov_in")][0])
        r = b.rec(600, [(50, _run(3 * lf_in + 1))])
        b.want("(c) run of the repeat unit: RC(R) between p1 + 1 and p1 + lf", "selfov_in", r, (0, 50, 0, 51))
        r = b.rec(300, [(50, _run(lf_in + 2))])
        b.want("(c) RC(R) inside F, an overlapping copy of F two bases on", "selfov_in", r, (0, 50, 0, 51))
    b.want("(d) palindromic F, R = F", "pal", b.rec(200, [(70, P)]), (0, 70, 0, 70))
    Fd, Rd = c.primers[c.pair("dege")]
    e, rc = iupac.expand(Fd), [iupac.revcomp(t) for t in iupac.expand(Rd)]
    lf, ld = len(Fd), len(Rd)
    r = b.rec(500, [(40, e[2]), (40 + lf + GAP, rc[0]), (300, e[1]), (300 + lf + GAP, rc[0])])
    b.want("(e) expansion 0 absent, 1 far right, 2 far left", "dege", r, (1, 300, 0, 300 + lf + GAP))
    r = b.rec(500, [(40, e[3]), (40 + lf + GAP, rc[0]), (400, e[0])])
    b.want("(f) expansion 0 without a reverse site, expansion 3 with one", "dege", r, (3, 40, 0, 40 + lf + GAP))
    r = b.rec(500, [(40, e[0]), (40 + lf + GAP, rc[1]), (40 + lf + GAP + ld + GAP, rc[0])])
    b.want("(g) reverse expansion 0 right of expansion 1", "dege", r, (0, 40, 0, 40 + lf + GAP + ld + GAP))
    for what, text in _mutants(f):
        b.want("(h) %s inside the forward site" % what, "main", b.rec(250, [(50, text), (x, rr)]), NONE)
    for what, text in _mutants(rr):
        b.want("(h) %s inside the reverse site" % what, "main", b.rec(250, [(50, f), (x, text)]), NONE)
    b.want("(h) lower-case product", "main", b.rec(250, [(50, (f + b.rnd(GAP) + rr).lower())]), NONE)
    r = b.rec(300, [(50, rr), (50 + lr + GAP, f)])
    b.want("(j) RC(R) of main, then F of main", "j", r, (0, 50, 0, 50 + lr + GAP))
    b.want("(j) RC(R) of main, then F of main", "main", r, NONE)
    for i in range(len(spec["extras"])):
        fx, rx = c.primers[c.pair("extra%d" % i)]
        r = b.rec(300, [(50, fx), (50 + len(fx) + GAP, iupac.revcomp(rx))])
        b.want("plain product", "extra%d" % i, r, (0, 50, 0, 50 + len(fx) + GAP))
    b.want("empty record last", "main", b.rec(0), NONE)
    # single-record database; 257 tiny records (a second block of the rolling kernel with one row in it)
    one = Call(group, group + "/single", {"main": (f, R)})
    r = _Builder(one, rng).rec(300, [(60, f), (60 + L + GAP, rr)])
    one.expect.append(("single-record database", "main", r, (0, 60, 0, 60 + L + GAP)))
    tiny = Call(group, group + "/tiny257", {"main": (f, R), "pal": (P, P)})
    bt = _Builder(tiny, rng)
    for i in range(257):
        if i % 16 == 0:
            bt.want("tiny record %d is a product" % i, "main", bt.rec(L + lr, [(0, f + rr)]), (0, 0, 0, L))
        elif i % 16 == 8:
            bt.want("tiny record %d is a palindromic site" % i, "pal", bt.rec(len(P), [(0, P)]), (0, 0, 0, 0))
        else:
            bt.want("tiny record %d" % i, "main", bt.rec(i % (L + lr)), NONE)
    return [c, one, tiny]


def _occ_calls(group, lengths, rng):
    """One pair per call, records of (F + spacer) repeated: the occurrence list holds exactly HITS - 1, HITS (served from the list),
    HITS + 1 and 6000 (the per-pair fall-back) entries.  By the rule the Product ends at the second F, so RC(R) behind the repeats
    is not found; two more records hold RC(R) inside the first Product, at HITS and HITS + 1 entries."""
    lf, lr = lengths
    for _ in range(1000):
        F = _plain(rng, lf)
        R = _plain(rng, lr, [F])
        rr = iupac.revcomp(R)
        sp = "".join(rng.choice(list("ACGT"), size=2))
        unit = F + sp
        probe = unit * 3 + rr + sp + unit * 2
        if occurrences(probe, [F, rr]) == 6:
            break
    c = Call(group, group + "/occurrences", {"occ": (F, R)})
    for n in OCC_COUNTS:
        c.records.append(unit * (n - 1) + rr)
        c.counts.append((len(c.records) - 1, n))
        c.expect.append(("%d occurrences, RC(R) behind the repeats" % n, "occ", len(c.records) - 1, NONE))
    for n in (HITS, HITS + 1):
        c.records.append(unit + rr + sp + unit * (n - 2))
        c.counts.append((len(c.records) - 1, n))
        c.expect.append(("%d occurrences, RC(R) in the first Product" % n, "occ", len(c.records) - 1, (0, 0, 0, len(unit))))
    c.planted = [np.ones(len(s), bool) for s in c.records]
    return [c]


def _degenerate(rng, n, twofold, used):
    s = _plain(rng, n, used)
    where = sorted(rng.choice(n, size=twofold, replace=False).tolist())
    for j in where:
        s = s[:j] + {"A": "RMW", "C": "YMS", "G": "RKS", "T": "YKW"}[s[j]][int(rng.integers(3))] + s[j + 1:]
    return s


def _table_calls(rng):
    """One database of 8 records of at most 195 bases, six calls: per primer length (20: one word, 40: two words) a table of exactly TABLE
    entries (the largest the block kernel takes), the same plus one plain pair (the whole call rolls), and one primer of TABLE
    expansions with a plain partner (TABLE + 1)."""
    pairs, used = {}, []
    for n in (20, 40):
        pairs["big%d" % n] = (_degenerate(rng, n, 11, used), _degenerate(rng, n, 11, used))
        pairs["plain%d" % n] = (_plain(rng, n, used), _plain(rng, n, used))
        pairs["one%d" % n] = (_degenerate(rng, n, 12, used), _plain(rng, n, used))
        used += [p for k in ("plain%d" % n, "one%d" % n) for p in pairs[k] if iupac.degeneracy(p) == 1]
    db = Call("G_table", "G_table/database", pairs)
    b = _Builder(db, rng)
    for n in (20, 40):
        F, R = pairs["big%d" % n]
        e, rc = iupac.expand(F), [iupac.revcomp(t) for t in iupac.expand(R)]
        F1, R1 = pairs["one%d" % n]
        e1 = iupac.expand(F1)
        Fp, Rp = pairs["plain%d" % n]
        assert len(e) == len(rc) == TABLE // 2 and len(e1) == TABLE
        g = 10                                   # short records: a thread of the rolling kernel walks a record once per expansion
        x, second = 5 + n + g, 5 + 2 * n + 2 * g
        y = second + n + g
        size = y + n + 5
        r = b.rec(size, [(5, e[2047]), (x, rc[2047]), (second, Fp), (y, iupac.revcomp(Rp))])
        b.want("the last expansions", "big%d" % n, r, (2047, 5, 2047, x))
        b.want("plain product", "plain%d" % n, r, (0, second, 0, y))
        r = b.rec(size, [(5, e[2047]), (x, rc[2046]), (second, e[5])])
        b.want("expansion 5 without a reverse site, 2047 with one", "big%d" % n, r, (2047, 5, 2046, x))
        r = b.rec(size, [(5, e1[4095]), (x, iupac.revcomp(R1))])
        b.want("the last expansion of %d" % TABLE, "one%d" % n, r, (4095, 5, 0, x))
        r = b.rec(size, [(5, e[1024]), (x, rc[0]), (second, e1[2048]), (y, iupac.revcomp(R1))])
        b.want("expansions 1024 and 0", "big%d" % n, r, (1024, 5, 0, x))
        b.want("expansion 2048 of %d" % TABLE, "one%d" % n, r, (2048, second, 0, y))
    assert len(db.records) == 8
    out = []
    for n in (20, 40):
        out += [db.sub("G_table/%d-table-of-4096" % n, ["big%d" % n]),
                db.sub("G_table/%d-table-of-4097" % n, ["big%d" % n, "plain%d" % n]),
                db.sub("G_table/%d-primer-of-4096" % n, ["one%d" % n])]
    return out


@functools.lru_cache(maxsize=None)
def calls(group):
    """The calls of one group, built once."""
    rng = np.random.default_rng([SEG, GROUP_NAMES.index(group)])
    if group == "G_table":
        return tuple(_table_calls(rng))
    out = _main_call(group, GROUPS[group], rng)
    if group in OCC_GROUPS:
        out += _occ_calls(group, OCC_GROUPS[group], rng)
    return tuple(out)


def table_size(call):
    return sum(iupac.degeneracy(p) for pr in call.primers for p in pr)


def unplanted(call):
    """(record, start, pattern) of every copy of a pattern of the call that is not inside the planted spans."""
    bad = []
    for r, s in enumerate(call.records):
        for p in set(patterns_of(call.primers)):
            bad += [(r, a, p) for a in _starts(s, p) if not call.planted[r][a:a + len(p)].all()]
    return bad


def encode(seqs):
    data = np.frombuffer("".join(seqs).encode(), np.uint8)
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return data, off


def encode_primers(primers):
    flat = [p for pr in primers for p in pr]
    codes = iupac.MASK_LUT[np.frombuffer("".join(flat).encode(), np.uint8)]
    off = np.zeros(len(flat) + 1, np.int32)
    np.cumsum([len(p) for p in flat], out=off[1:])
    return codes, off
