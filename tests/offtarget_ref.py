"""The off-target screen of include/mprime_offtarget.h restated on strings: the hit rule of include/mprime.h (mp_kmm_scan), the site
reduction, the sequence order and the amplicon rule, in plain Python and numpy.  The checker of tests/test_offtarget_edges.py; a
helper, not a test.  Nothing of multiprime_amd is used but iupac.MASK_LUT (for `encode`); the class joins go through tests/panel_ref.py.

A read hits row T at the 0-based start p on strand 0 when T[p : p + L] upper-cased differs from the read in at most `budget` columns
(a text base outside A/C/G/T differs from everything) and the last `term` columns all match; on strand 1 the same with the read's
reverse complement — both strands in text orientation, the trailing run counted from the window's last column downwards."""
from bisect import bisect_left

import numpy as np

import panel_ref
from multiprime_amd import iupac

_COMP = str.maketrans("ACGT", "TGCA")
COUNTS = ("hits", "forward_sites", "reverse_sites", "products", "forward_genes", "reverse_genes", "both_genes")


def rc(s):
    return s.translate(_COMP)[::-1]


def encode(strings):
    """(codes, offsets) of concrete reads as the library takes them."""
    codes = iupac.MASK_LUT[np.frombuffer("".join(strings).encode(), np.uint8)]
    off = np.zeros(len(strings) + 1, np.int32)
    np.cumsum([len(s) for s in strings], out=off[1:])
    return codes, off


def _text(seq):
    return np.frombuffer(seq.upper().encode(), np.uint8)


def hits(seqs, read, budget, term):
    """[(row, start, strand)] of one read, ascending."""
    m, out = len(read), []
    for strand, q in enumerate((read, rc(read))):
        q = np.frombuffer(q.encode(), np.uint8)
        for row, seq in enumerate(seqs):
            if len(seq) < m:
                continue
            differ = np.lib.stride_tricks.sliding_window_view(_text(seq), m) != q          # [start][column]
            n_mm = differ.sum(axis=1)
            run = np.where(n_mm > 0, np.argmax(differ[:, ::-1], axis=1), m)                 # matching columns behind the last mismatch
            out.extend((row, int(p), strand) for p in np.nonzero((n_mm <= budget) & (run >= term))[0])
    return sorted(out)


def sites_of(seqs, reads, budgets, term):
    """(per read its hit list, winners {(strand, row, position): largest read index that hits there},
    row_min {row: smallest read index with a forward hit})."""
    per_read = [hits(seqs, r, b, term) for r, b in zip(reads, budgets)]
    winners, row_min = {}, {}
    for i, hl in enumerate(per_read):                  # ascending read index: a later read overwrites, the first forward read stays
        for row, p, strand in hl:
            winners[(strand, row, p)] = i
            if strand == 0:
                row_min.setdefault(row, i)
    return per_read, winners, row_min


def by_row(winners, strand, ids):
    """{row: {position: id of the winning read}} of one strand."""
    out = {}
    for (s, row, p), i in winners.items():
        if s == strand:
            out.setdefault(row, {})[p] = ids[i]
    return out


def row_products(forward, reverse, lo, hi):
    """One row, forward / reverse = {position: primer}: [(start, stop, F, R, length)] by the header's words."""
    starts, stops = sorted(forward), sorted(reverse)
    if stops[0] - starts[-1] > hi or stops[-1] - starts[0] < lo:
        return []                                      # the whole row gives nothing
    out = []
    for a in starts:
        partners = stops[bisect_left(stops, a + lo):bisect_left(stops, a + hi)]     # the stops in [a + lo, a + hi)
        if not partners:
            break                                      # the first dead start ends the row
        for b in partners:
            if lo < b - a + 1 < hi:
                out.append((a, b, forward[a], reverse[b], b - a + 1))
    return out


def plain_filter(forward, reverse, lo, hi):
    """What a join WITHOUT the two cuts would give for the row: every pair with lo < length < hi (for the property tests)."""
    return [(a, b, forward[a], reverse[b], b - a + 1) for a in sorted(forward) for b in sorted(reverse) if lo < b - a + 1 < hi]


def row_order(row_min):
    return [row for _, row in sorted((i, row) for row, i in row_min.items())]


def screen(seqs, reads, read_primer, budgets, term, lo, hi):
    """(products [(row, start, stop, F, R, length)] in the order of the report, counts as mp_offtarget_stats names them)."""
    return screen_of(sites_of(seqs, reads, budgets, term), read_primer, lo, hi)


def screen_of(reduced, read_primer, lo, hi):
    """screen() on what sites_of() returned."""
    per_read, winners, row_min = reduced
    forward, reverse = by_row(winners, 0, read_primer), by_row(winners, 1, read_primer)
    products = []
    for row in row_order(row_min):
        if row in reverse:
            products.extend((row,) + p for p in row_products(forward[row], reverse[row], lo, hi))
    counts = (sum(map(len, per_read)), sum(map(len, forward.values())), sum(map(len, reverse.values())), len(products),
              len(forward), len(reverse), len(set(forward) & set(reverse)))
    return products, dict(zip(COUNTS, counts))


def screen_classes(seqs, reads, read_id, read_class, budgets, term, lo, hi):
    """mp_offtarget_classes: the reduction per (class, strand), the three joins of panel_ref.join_classes with rows ascending.
    (products [(row, start, stop, F, R, length, join class)], counts: the hits of every read, and the sites, products and rows summed
    over the joins that have sites on both of their sides — the library runs no other)."""
    per_read = [hits(seqs, r, b, term) for r, b in zip(reads, budgets)]
    winners = {}
    for i, hl in enumerate(per_read):
        for row, p, strand in hl:
            winners[(read_class[i], strand, row, p)] = i
    sites = [(cls, strand, row, p, read_id[i]) for (cls, strand, row, p), i in sorted(winners.items())]
    products = panel_ref.join_classes(sites, lo, hi)
    counts = [sum(map(len, per_read)), 0, 0, len(products), 0, 0, 0]
    for fc, rcl in panel_ref.JOINS:
        f = {(row, p) for cls, strand, row, p, _ in sites if (cls, strand) == (fc, 0)}
        r = {(row, p) for cls, strand, row, p, _ in sites if (cls, strand) == (rcl, 1)}
        if f and r:
            f_rows, r_rows = {row for row, _ in f}, {row for row, _ in r}
            for k, v in ((1, len(f)), (2, len(r)), (4, len(f_rows)), (5, len(r_rows)), (6, len(f_rows & r_rows))):
                counts[k] += v
    return products, dict(zip(COUNTS, counts))
