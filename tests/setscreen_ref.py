"""The rule of include/mprime_setscreen.h in plain Python: the checker of the set screen (csrc/setscreen.hip) and of the greedy
logic around it (multiprime_amd/maxset.py -r).  Nothing here is shared with the code under test except iupac.expand (the
reference's own expansion order) and test_validate.brute, the string statement of mp_kmm_scan's acceptance rule."""
from multiprime_amd import iupac
from test_validate import brute

TERM_MATCH = 5


def reads_of(primer, dist):
    term = primer if dist == 0 or len(primer) <= dist else primer[-dist:]
    return iupac.expand(term)


def sites(background, primers, dist, m, term=TERM_MATCH):
    """{primer: (forward, reverse)}: the SETS of (row, pos) at which at least one read of the primer hits on strand 0 / 1."""
    out = {}
    for p in dict.fromkeys(primers):
        hits = brute(background, reads_of(p, dist), m, term)
        out[p] = ({(r, pos) for r, pos, _, s in hits if s == 0}, {(r, pos) for r, pos, _, s in hits if s == 1})
    return out


def products_of_sites(fwd, rev, lo, hi):
    """the double loop of the rule: forward sites x reverse sites of one row with lo < stop - start + 1 < hi"""
    n = 0
    for ra, pa in fwd:
        for rb, pb in rev:
            if ra == rb and lo < pb - pa + 1 < hi:
                n += 1
    return n


def pair_table(site_map, lo, hi):
    """{(A, B): products(A -> B)} over all ordered pairs, zero counts left out"""
    table = {}
    for a, (fa, _) in site_map.items():
        for b, (_, rb) in site_map.items():
            n = products_of_sites(fa, rb, lo, hi)
            if n:
                table[(a, b)] = n
    return table


def own_cross(table, f, r, selected):
    new = {f, r}
    own = sum(table.get((a, b), 0) for a in new for b in new)
    cross = sum(table.get((a, b), 0) + table.get((b, a), 0) for a in new for b in set(selected) - new)
    return own, cross


def triples(table, ids):
    """the table as sorted (A id, B id, count) triples"""
    return sorted((ids[a], ids[b], n) for (a, b), n in table.items())
