"""Plain restatement of the rule of include/mprime_dege.h — the yardstick of tests/test_dege_gpu.py, checked itself by tests/test_dege.py
against tables recorded from the unmodified DegePrime.pl and against an exhaustive search.  No numpy: lists, dicts, ints and the standard library."""
import bisect
import functools
import itertools
import math
import re

LETTERS = "ACGT"
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "AC": "M", "AG": "R", "AT": "W", "CG": "S", "CT": "Y", "GT": "K", "ACG": "V", "ACT": "H",
         "AGT": "D", "CGT": "B", "ACGT": "N"}
IUPAC_SET = {v: k for k, v in IUPAC.items()}
MASK = (1 << 64) - 1
MAX_DRAWS = 100
HEADER = "Pos\tNumberSpanning\tUniqueMers\tEntropy\tPrimerDeg\tPrimerSeq\tNumberMatching\tFractionMatching"


def read_fasta(text):
    """[(id, sequence)] as DegePrime.pl reads them: the id is the first token of the '>' line, rows are joined."""
    out = []
    for line in text.splitlines():
        if line.startswith(">"):
            f = line.split()
            out.append([f[0][1:] if f else "", []])
        elif out:
            out[-1][1].append(line)
    return [(i, "".join(s)) for i, s in out]


def is_letter(ch):
    return ch not in "-."


def extent(row):
    """(start, end): first and last letter; an all-gap row gives (len, -1)."""
    start = next((i for i, ch in enumerate(row) if is_letter(ch)), len(row))
    end = next((i for i in range(len(row) - 1, -1, -1) if is_letter(row[i])), -1)
    return start, end


def valid_degeneracy(d):
    """The largest value <= d of the form 2^a 3^b."""
    def ok(x):
        while x % 2 == 0:
            x //= 2
        while x % 3 == 0:
            x //= 3
        return x == 1
    while not ok(d):
        d -= 1
    return d


def word_of(mer):
    w = 0
    for ch in mer:
        w = (w << 2) | LETTERS.index(ch)
    return w


def mer_of(word, l):
    return "".join(LETTERS[(word >> (2 * (l - 1 - p))) & 3] for p in range(l))


def entropy_of(counts, n):
    """counts: the count of every distinct mer of the spanning rows.  Summed per count value in ascending order, the multiplicity
    multiplied in — the order mprime_dege.h fixes."""
    mult = {}
    for c in counts:
        mult[c] = mult.get(c, 0) + 1
    e = 0.0
    for c in sorted(mult):
        x = c / n
        e = e - mult[c] * (x * math.log(x) / math.log(2))
    return e


def window(rows, extents, pos, l, skip):
    """(NumberSpanning, Z, entropy, [(word, count)] ascending) of one window."""
    all_mers, free = {}, {}
    n = z = 0
    for row, (start, end) in zip(rows, extents):
        if start + skip <= pos and end - skip >= pos + l - 1:
            mer = row[pos:pos + l - 1] + row[pos + l - 1].upper()
            n += 1
            all_mers[mer] = all_mers.get(mer, 0) + 1
            if all(ch in LETTERS for ch in mer):
                z += 1
                free[mer] = free.get(mer, 0) + 1
    uniq = sorted((word_of(m), c) for m, c in free.items())
    return n, z, entropy_of(all_mers.values(), n) if n else 0.0, uniq


def windows(rows, l, skip=20):
    ext = [extent(r) for r in rows]
    width = len(rows[0])
    return [window(rows, ext, pos, l, skip) for pos in range(width - l + 1)]


def mix(z):
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    z ^= z >> 31
    return z


def draw(seed, pos, it, t, r):
    n = pos * (1 << 24) + it * (1 << 8) + t
    u = mix(seed + (n + 1) * 0x9E3779B97F4A7C15) >> 32
    return (u * r) >> 32


BIT = {"A": 1, "C": 2, "G": 4, "T": 8}
SIZE = [bin(m).count("1") for m in range(16)]
SET_OF = ["".join(ch for ch in LETTERS if m & BIT[ch]) for m in range(16)]


def iteration(uniq, l, max_deg, seed, pos, it, mers=None):
    """(deg, match, n_draws, sets) of one iteration; sets[p] is a sorted string of letters.  A set is kept as four bits; the remaining
    mers' running sums are rebuilt for every draw and searched; the final count is a regular expression over the mers."""
    mers = mers or [mer_of(w, l) for w, _ in uniq]
    sets = [0] * l
    deg, n_draws = 0, 0
    remaining = list(range(len(uniq)))
    total = sum(c for _, c in uniq)
    for t in range(MAX_DRAWS):
        if deg >= max_deg or total == 0:
            break
        r = draw(seed, pos, it, t, total)
        sums = list(itertools.accumulate(uniq[i][1] for i in remaining))
        k = bisect.bisect_right(sums, r)       # the first running sum that exceeds r
        i = remaining.pop(k)
        total -= uniq[i][1]
        n_draws += 1
        union = [sets[p] | BIT[ch] for p, ch in enumerate(mers[i])]
        newdeg = 1
        for m in union:
            newdeg *= SIZE[m]
        if newdeg <= max_deg:
            deg, sets = newdeg, union
    if all(sets):
        rx = _pattern("".join("[%s]" % SET_OF[m] for m in sets))
        match = sum(c for mer, (_, c) in zip(mers, uniq) if rx.fullmatch(mer))
    else:
        match = 0
    return deg, match, n_draws, [SET_OF[m] for m in sets]


@functools.lru_cache(maxsize=4096)
def _pattern(text):
    return re.compile(text)


def merge(uniq, l, max_deg, iters, seed, pos):
    """Every iteration of a window and the index of the winner (the largest match, the earliest among equals)."""
    mers = [mer_of(w, l) for w, _ in uniq]
    its = [iteration(uniq, l, max_deg, seed, pos, it, mers) for it in range(iters)]
    best = 0
    for k, x in enumerate(its):
        if x[1] > its[best][1]:
            best = k
    return its, best


def fmt(x):
    """Perl's stringification of a number: %.15g, never -0."""
    s = "%.15g" % x
    return "0" if s == "-0" else s


def table_rows(rows, l, max_deg, skip=20, depth=1, iters=100, seed=0):
    """The table as a list of rows of strings (no header)."""
    out = []
    for pos, (n, z, ent, uniq) in enumerate(windows(rows, l, skip)):
        if z < depth:
            continue
        its, best = merge(uniq, l, max_deg, iters, seed, pos)
        deg, match, _, sets = its[best]
        out.append([str(pos), str(n), str(len(uniq)), fmt(ent), str(deg), "".join(IUPAC[s] for s in sets), str(match), fmt(match / n)])
    return out


def table_text(rows, l, max_deg, **kw):
    return HEADER + "\n" + "".join("\t".join(r) + "\n" for r in table_rows(rows, l, max_deg, **kw))


def recount(primer, uniq, l):
    """The rows among the gap-free ones that a degenerate oligomer matches."""
    return sum(c for w, c in uniq if all(ch in IUPAC_SET[primer[p]] for p, ch in enumerate(mer_of(w, l))))


def optimum(uniq, l, max_deg):
    """The best match any oligomer of degeneracy <= max_deg reaches: exhaustive over the non-empty letter sets per position, restricted
    to the letters that occur there (another letter adds degeneracy and matches nothing)."""
    seen = [sorted({mer_of(w, l)[p] for w, _ in uniq}) for p in range(l)]
    choices = []
    for p in range(l):
        subs = []
        for m in range(1, 1 << len(seen[p])):
            subs.append("".join(ch for k, ch in enumerate(seen[p]) if m >> k & 1))
        choices.append(subs)
    best = 0

    def walk(p, deg, alive):
        nonlocal best
        if p == l:
            best = max(best, sum(c for _, c in alive))
            return
        for s in choices[p]:
            if deg * len(s) <= max_deg:
                nxt = [(m, c) for m, c in alive if m[p] in s]
                if nxt:
                    walk(p + 1, deg * len(s), nxt)
    walk(0, 1, [(mer_of(w, l), c) for w, c in uniq])
    return best
