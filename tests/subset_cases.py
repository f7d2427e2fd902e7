"""Constructed inputs of the subset search (include/mprime_subset.h), the smallest that can break each path of csrc/subset.hip.  A case is
    {"name", "k", "v", "N", "windows": [[(k-mer, count), ...], ...], "searches": [(window, seed, cover_number), ...]}
with k-mers over A, C, G, T and '-'.  tests/test_subset_gpu.py runs every case through the explicit form and compares each per-step result,
the replayed subset, count and primer with tests/subset_ref.py.

Sizes the kernels branch on: 256 records per LDS tile; 1024 ranks per workgroup (256 lanes x 4 ranks); 64 lanes per wave; elements 0..63
in the low word of a mask and 64..127 in the high one.  No C(t, m) with t <= 128 and m >= 2 equals 1024, so "a rank count at the number of
ranks one workgroup takes" is met by the pass over the ranks below an early exit at rank 1024 (case exit_at_1024); C(14, 4) = 1001 and
C(46, 2) = 1035 are the counts just below and above.
"""
import random
from itertools import combinations, islice

BASES = "ACGT"


def sub(seed, changes):
    s = list(seed)
    for pos, base in changes:
        s[pos] = base
    return "".join(s)


def alt(seed, pos, j):
    """The j-th base (0..2) other than the seed's at pos."""
    return [b for b in BASES if b != seed[pos]][j]


def elements(seed, n, positions=None):
    """n distinct (position, base != seed) elements, base-major so that neighbours in the list sit at different positions."""
    positions = list(range(len(seed))) if positions is None else positions
    out = [(p, alt(seed, p, j)) for j in range(3) for p in positions]
    assert n <= len(out)
    return out[:n]


def elements65(seed):
    """65 elements of a 24-base seed whose first two and last two in (position, base) order sit at different positions — so that the
    first and the last combination of two can be one record: one base at positions 0 and 23, three at 1..21, none at 22."""
    mid = list(range(1, 22))
    return [(0, alt(seed, 0, 0))] + [(p, alt(seed, p, 0)) for p in mid] + [(23, alt(seed, 23, 0))] + [(p, alt(seed, p, j)) for j in (1, 2) for p in mid]


def case(name, k, v, N, windows, searches):
    for w in windows:
        assert all(len(u) == k for u, _ in w), name
    return {"name": name, "k": k, "v": v, "N": N, "windows": windows, "searches": searches}


def random_window(rng, seed, n_rec, pool, max_y, with_seed=True, gaps=False):
    """n_rec distinct k-mers that differ from the seed at 1..max_y positions of `pool`, counts 1..40."""
    seen, out = set(), []
    if with_seed:
        out.append((seed, rng.randint(1, 90)))
        seen.add(seed)
    while len(out) < n_rec + (1 if with_seed else 0):
        pos = rng.sample(pool, rng.randint(1, min(max_y, len(pool))))
        u = sub(seed, [(p, "-" if gaps and rng.random() < 0.15 else alt(seed, p, rng.randrange(3))) for p in pos])
        if u not in seen:
            seen.add(u)
            out.append((u, rng.randint(1, 40)))
    rng.shuffle(out)
    return out


def total(window):
    return sum(n for _, n in window)


def random_seed(rng, k):
    return "".join(rng.choice(BASES) for _ in range(k))


def grid_cases():
    """k = 4, 31, 32 (element ids 124..127 in use at 32) x v = 0, 1, 2 x N = 1, 2, 4, 6."""
    out = []
    for k in (4, 31, 32):
        for v in (0, 1, 2):
            for N in (1, 2, 4, 6):
                rng = random.Random(1000 * k + 10 * v + N)
                seed = random_seed(rng, k)
                pool = list(range(4)) if k == 4 else [0, 7, 15, 16, k - 2, k - 1]
                w = random_window(rng, seed, 10 if k == 4 else 30, pool, 4, gaps=(v > 0))
                if k == 32:
                    w.append((sub(seed, [(31, alt(seed, 31, 2)), (30, alt(seed, 30, 1))]), 5))
                out.append(case(f"grid_k{k}_v{v}_N{N}", k, v, N, [w], [(0, seed, total(w))]))
    return out


def pair_records(seed, elems, count=1):
    """Records of two elements each, neighbours of the list (the last one wraps), so that T = elems exactly."""
    out = []
    for i in range(0, len(elems), 2):
        a, b = elems[i], elems[(i + 1) % len(elems)]
        assert a[0] != b[0]
        out.append((sub(seed, [a, b]), count))
    return out


def rank_pair(t, rank):
    return next(islice(combinations(range(t), 2), rank, rank + 1))


def edge_cases():
    out = []
    seed8 = "AAAAAAAA"
    # degenerate inputs
    out.append(case("only_the_seed", 8, 1, 4, [[(seed8, 9)]], [(0, seed8, 9)]))
    out.append(case("empty_window", 8, 1, 3, [[]], [(0, seed8, 1)]))
    out.append(case("one_admitted_record", 8, 1, 4, [[(seed8, 3), ("CCAAAAAA", 2), ("CAAAAAAA", 4)]], [(0, seed8, 9)]))
    out.append(case("all_records_one_element", 8, 1, 4, [[(seed8, 3), ("CAAAAAAA", 2), ("AGAAAAAA", 4), ("AAAAAAAT", 1)]], [(0, seed8, 10)]))
    # record counts at the LDS tile: two-element records over 12 positions (594 to choose from), N = 3
    seed31 = random_seed(random.Random(31), 31)
    pos12 = list(range(0, 31, 3))[:12]
    two = [sub(seed31, [(a, alt(seed31, a, i)), (b, alt(seed31, b, j))]) for a, b in combinations(pos12, 2) for i in range(3) for j in range(3)]
    rng = random.Random(256)
    rng.shuffle(two)
    for n in (255, 256, 257, 513):
        w = [(u, rng.randint(1, 9)) for u in two[:n]]
        out.append(case(f"tile_{n}_records", 31, 1, 3, [w], [(0, seed31, total(w) + 5)]))
    # |T| across the dn threshold
    e3 = elements(seed8, 3, [0, 1, 2])
    out.append(case("T_is_dn_minus_1", 8, 1, 4, [[(sub(seed8, e3[:2]), 2), (sub(seed8, e3[1:]), 3)]], [(0, seed8, 6)]))        # |T| = 3 < 4 at dn = 4
    e4 = elements(seed8, 4, [0, 1, 2, 3])
    out.append(case("T_is_dn", 8, 1, 4, [[(sub(seed8, e4[:2]), 2), (sub(seed8, e4[2:]), 3), (sub(seed8, e4[1:3]), 1)]], [(0, seed8, 7)]))
    # |T| = 64 and 65: the wave width, and more than one workgroup of ranks at N = 3 (C(65, 2) = 2080)
    seed24 = random_seed(random.Random(24), 24)
    e65 = elements65(seed24)
    for t in (64, 65):
        w = pair_records(seed24, e65[:t], 1)
        w[3] = (w[3][0], 4)
        out.append(case(f"T_{t}", 24, 0, 3, [w], [(0, seed24, 1000)]))
    # rank counts around the 1024 ranks of one workgroup
    seed16 = random_seed(random.Random(16), 16)
    w = pair_records(seed16, elements(seed16, 14), 2) + [(sub(seed16, elements(seed16, 14)[4:8]), 3)]
    out.append(case("ranks_1001", 16, 1, 5, [w], [(0, seed16, 500)]))                # C(14, 4) at dn = 5
    w = pair_records(seed16, elements(seed16, 46), 2)
    out.append(case("ranks_1035", 16, 0, 3, [w], [(0, seed16, 500)]))                # C(46, 2) at dn = 3
    # The optimum at rank 0 and at the last rank; equal totals in two workgroups (ranks 10 and 1500 of 2080): the lower one wins, also
    # with the entries in another order.  v = 0: a combination's total is the count of the one record it equals.  Step 2 admits nothing
    # and sets max_count = cover_number = 1; the background records count 2, so no total is 1 and step 3's best replaces the subset.
    base = pair_records(seed24, e65, 2)
    sorted65 = sorted(range(65), key=lambda i: (e65[i][0], BASES.index(e65[i][1])))      # rank order is the order of the SORTED elements

    def heavy(rank, count):
        a, b = rank_pair(65, rank)
        a, b = e65[sorted65[a]], e65[sorted65[b]]
        assert a[0] != b[0], (rank, a, b)
        return (sub(seed24, [a, b]), count)

    def distinct(window):
        seen = {}
        for u, n in window:
            seen[u] = seen.get(u, 0) + n
        return list(seen.items())

    out.append(case("optimum_at_rank_0", 24, 0, 3, [distinct(base + [heavy(0, 50)])], [(0, seed24, 1)]))
    out.append(case("optimum_at_last_rank", 24, 0, 3, [distinct(base + [heavy(2079, 50)])], [(0, seed24, 1)]))
    ties = base + [heavy(10, 50), heavy(1500, 50)]
    assert len(distinct(ties)) == len(ties)
    out.append(case("equal_totals_two_workgroups", 24, 0, 3, [ties], [(0, seed24, 1)]))
    out.append(case("equal_totals_two_workgroups_permuted", 24, 0, 3, [ties[::-1]], [(0, seed24, 1)]))
    # early exits: at the first rank; after lower ranks set max_count; at a later step after an earlier one set a subset; at rank 1024 of
    # 2080 (the pass over the ranks below it is exactly one workgroup), and at rank 1025
    out.append(case("exit_first_rank", 8, 1, 3, [[("CCAAAAAA", 1), ("CACAAAAA", 1)]], [(0, seed8, 2)]))
    out.append(case("exit_after_lower_ranks", 8, 1, 3, [[("ACCAAAAA", 1), ("AACCAAAA", 1), ("CACAAAAA", 1)]], [(0, seed8, 3)]))
    out.append(case("exit_at_a_later_step", 8, 1, 4, [[("CCAAAAAA", 1), ("AACCAAAA", 1), ("CACACAAA", 1)]], [(0, seed8, 3)]))
    for rank in (1024, 1025):
        w = distinct(base + [heavy(rank, 7)])
        out.append(case(f"exit_at_{rank}", 24, 0, 3, [w], [(0, seed24, dict(w)[heavy(rank, 7)[0]])]))
    # gap elements count as a mismatch and merge to nothing; a k-mer with more gaps than v is no record at all
    out.append(case("gap_elements", 8, 1, 3, [[("-CGTACGA", 1), ("CCGTACGA", 1), ("--GTACGA", 9)]], [(0, "ACGTACGT", 2)]))
    out.append(case("gap_elements_v2", 8, 2, 4, [[("-CGTAC-A", 3), ("CCGTACGA", 1), ("AC-TACGA", 2), ("ACGTACGT", 4)]], [(0, "ACGTACGT", 10)]))
    # a seed that is no key of the table, beside one that is
    w = random_window(random.Random(5), "ACGTACGTAC", 25, [1, 3, 5, 7, 9], 3, with_seed=False)
    out.append(case("seed_not_a_key", 10, 1, 4, [w], [(0, "ACGTACGTAC", total(w)), (0, w[0][0], total(w))]))
    # NM != MM with equal counts: NM wins (searches 0 and 1 are the NM and the MM seed of one window)
    out.append(case("nm_mm_tie", 8, 1, 2, [[("AAAAAAAA", 5), ("CCAAAAAA", 5)]], [(0, "AAAAAAAA", 10), (0, "CCAAAAAA", 10)]))
    # counts near 2^31: a total of 2^32 - 4
    out.append(case("counts_near_2_31", 8, 1, 3, [[("CCAAAAAA", 2 ** 31 - 1), ("CACAAAAA", 2 ** 31 - 3), ("AAAAAAAA", 2)]], [(0, seed8, 2 ** 32 - 2)]))
    return out


def ragged_case():
    """33 searches of different |T| and record counts in one call (k = 18, v = 1, N = 4), two of them on one window."""
    rng = random.Random(33)
    windows, searches = [], []
    for i in range(32):
        seed = random_seed(rng, 18)
        pool = rng.sample(range(18), 2 + i % 6)
        w = random_window(rng, seed, min((i * 7) % 45, 3 ** min(len(pool), 3)), pool, 4, with_seed=i % 3 != 0, gaps=i % 5 == 0)
        windows.append(w)
        searches.append((i, seed, total(w) + (i % 2)))
    searches.append((7, windows[7][0][0], total(windows[7])))
    return case("ragged_33_searches", 18, 1, 4, windows, searches)


def all_cases():
    return grid_cases() + edge_cases() + [ragged_case()]


def refusal_cases():
    """(case, fragment of the message)."""
    seed33 = "A" * 33
    seed24 = random_seed(random.Random(24), 24)
    return [
        (case("k_33", 33, 1, 3, [[(seed33, 1)]], [(0, seed33, 1)]), "at most 32"),
        (case("combinations_beyond_32_bits", 24, 0, 9, [pair_records(seed24, elements65(seed24), 1)], [(0, seed24, 100)]), "more than 32 bits"),
        (case("counts_beyond_32_bits", 8, 1, 3, [[("CCAAAAAA", 2 ** 31), ("CACAAAAA", 2 ** 31)]], [(0, "AAAAAAAA", 2 ** 32)]), "exceed 32 bits"),
    ]
