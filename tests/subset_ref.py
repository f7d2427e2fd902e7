"""Plain-Python model of the global-optimum degenerate positions (`-m multiPrime2`): strings, sets and itertools, nothing shared with
the product and nothing taken from the reference's text.  The rules (per seed of a window):

  records   every key u of `cover` other than the seed gives (Y(u), cover[u]) with Y(u) = {(i, b)} over the positions i where
            u[i] != seed[i]; b = u[i], and b = seed[i] where u[i] is a gap (the element counts as a mismatch, merging it changes nothing).
  steps     max_count = 0, subset = {}; for dn = 2 .. N: the records with 1 < |Y| < dn + v are admitted, T = the union of their elements.
            |T| >= dn: the combinations S of dn - 1 elements of T, in lexicographic order of the elements sorted by (position, A<C<G<T),
                       each get total = sum of the counts of the admitted records with |Y - S| <= v;
                       a total equal to cover_number ends the whole search with (max_count as it stands, S);
                       a total strictly above max_count replaces (max_count, subset) — so the first maximum wins.
            |T| <  dn: max_count = cover_number, subset = T, and the loop goes on.
  merge     every element (i, b) of the subset adds b to the IUPAC set at position i of the seed.
  NM or MM  NM wins when its max_count >= MM's.
"""
from itertools import combinations

BASES = "ACGT"
IUPAC = {frozenset("A"): "A", frozenset("C"): "C", frozenset("G"): "G", frozenset("T"): "T", frozenset("AG"): "R", frozenset("CT"): "Y",
         frozenset("AC"): "M", frozenset("GT"): "K", frozenset("CG"): "S", frozenset("AT"): "W", frozenset("ACT"): "H", frozenset("CGT"): "B",
         frozenset("ACG"): "V", frozenset("AGT"): "D", frozenset("ACGT"): "N"}


def elements(seed, u):
    """Y(u): a frozenset of (position, base)."""
    return frozenset((i, seed[i] if c == "-" else c) for i, c in enumerate(u) if c != seed[i])


def records(seed, cover_items):
    """[(Y, count)] of every key other than the seed, in the order given."""
    return [(elements(seed, u), n) for u, n in cover_items if u != seed]


def element_key(e):
    return (e[0], BASES.index(e[1]))


def step(recs, dn, v, cover_number):
    """One step on its own: (T sorted, number of admitted records, best total, its lowest rank, lowest rank whose total equals cover_number,
    best total over the ranks below that one).  Ranks are -1 and totals 0 where |T| < dn or nothing applies."""
    adm = [(y, n) for y, n in recs if 1 < len(y) < dn + v]
    T = sorted(set().union(*[y for y, _ in adm]) if adm else set(), key=element_key)
    best, best_rank, exit_rank, pre = 0, -1, -1, 0
    if len(T) >= dn:
        for rank, S in enumerate(combinations(T, dn - 1)):
            chosen = set(S)
            total = sum(n for y, n in adm if len(y - chosen) <= v)
            if total == cover_number:
                exit_rank = rank
                break
            if best_rank < 0 or total > best:
                best, best_rank = total, rank
        if exit_rank >= 0:
            pre = best if best_rank >= 0 else 0
            # the best over ALL ranks, as the device reports it (the exit rank's total is cover_number)
            best, best_rank = 0, -1
            for rank, S in enumerate(combinations(T, dn - 1)):
                chosen = set(S)
                total = sum(n for y, n in adm if len(y - chosen) <= v)
                if best_rank < 0 or total > best:
                    best, best_rank = total, rank
    return T, len(adm), best, best_rank, exit_rank, pre


def select(seed, cover_items, cover_number, N, v):
    """(subset as a sorted list of (position, base), max_count, merged primer) — the whole search of one seed."""
    recs = records(seed, cover_items)
    max_count, subset = 0, []
    for dn in range(2, N + 1):
        adm = [(y, n) for y, n in recs if 1 < len(y) < dn + v]
        T = sorted(set().union(*[y for y, _ in adm]) if adm else set(), key=element_key)
        if len(T) >= dn:
            done = False
            for S in combinations(T, dn - 1):
                chosen = set(S)
                total = sum(n for y, n in adm if len(y - chosen) <= v)
                if total == cover_number:
                    subset, done = list(S), True
                    break
                if total > max_count:
                    max_count, subset = total, list(S)
            if done:
                break
        else:
            max_count, subset = cover_number, list(T)
    return sorted(subset, key=element_key), max_count, merge(seed, subset)


def merge(seed, subset):
    sets = [set(c) for c in seed]
    for i, b in subset:
        sets[i].add(b)
    return "".join(IUPAC[frozenset(s)] for s in sets)


def pick(nm, mm):
    """nm, mm = (subset, max_count, primer) of the two seeds (mm None: one seed); NM wins ties."""
    return nm if mm is None or nm[1] >= mm[1] else mm


def mask_of(elems):
    """The element set as the library's 128-bit mask (low word, high word): element id = 4 * position + base index."""
    m = 0
    for i, b in elems:
        m |= 1 << (4 * i + BASES.index(b))
    return m & (2 ** 64 - 1), m >> 64
