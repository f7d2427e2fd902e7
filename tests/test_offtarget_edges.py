"""The off-target screen behind its scan (multiprime_amd/csrc/offtarget.hip and the sink of csrc/kmm.hpp) at its edges: the site map
(atomicMax of read + 1 across one launch per budget), the per-sequence row_min (forward hits only), the compaction (map_count_kernel,
scan_i64, map_write_kernel), site_rows_kernel / row_of over offsets that tie at empty records, the join on store-offset keys
(join_count / join_cut / join_rows / join_emit, sequences by (row_min, sequence)), the kept products of a repeated call, the four-segment
map of mp_offtarget_classes and the entry of mp_offtarget_gap_resident that admits no gap.  Against tests/offtarget_ref.py, a model of
the whole screen on strings; the inputs are those of tests/offtarget_cases.py.

CPU leg: the model's hits equal the checker's resident scan per budget, its per-row join equals validate.amplicons() (and
panel_ref.join), and every case contains what it is built for, asserted on the model.  GPU leg (`-m gpu`): products in order and all seven
counts of mp_offtarget_stats equal the model's.  Every comparison is equality of integer tuples.

What each case reaches, from the constants of the code (a chunk of the compaction is kBlock * 16 = 4096 map entries in 16 rounds of
256, a scan tile kBlock * 8 = 2048 elements, a scan workgroup kSeg = 8192 starts of one record, the join one thread per forward site
or per record in blocks of 256; a table goes through the two-word kernel when its longest read has more than 32 bases):
  a1     49610 bases in 14 records, 17 scan workgroups; budgets 0 {S4} and 1 {PAL} one-word, 2 {S33, S32, S31} and 3 {S64, S63} two-word:
         four launches into one map; map of 99220 entries = 25 chunks (the last of 916 entries), the strands meet inside chunk 12; one
         scan tile; a few hundred forward sites: two blocks of the join.  a1rev: the same launches, other read indices.
  a2     budgets 1 {S33 .. S4} and 2 {S64, S63}, both two-word (the 4-base read rides on the two-word table): two launches; term 4.
  a3     budgets 1 {PAL, S4} one-word, 2 and 3 two-word: three launches; thousands of sites per strand: more than one scan tile of
         the join's counts, more than ten blocks of the join.
  b      8226 bases, 3 scan workgroups, one two-word launch; map of 16452 entries = 5 chunks (the last of 68), every round of the
         forward half full but the one holding a record's last three bases; 8220 forward sites = 5 scan tiles (the last of 28) and
         33 blocks of the join (the last of 28 sites).
  c      8191 / 8192 / 8193 bases in 8 records (4 of them empty, one of 3 bases), one one-word launch; map of 16382 (4 chunks, the
         last short by two), 16384 (4 whole chunks) and 16386 entries (5 chunks, the last of two); the reverse half starts at entry
         8191 (the last of chunk 1), 8192 (the first of chunk 2) and 8193; sites at entries 0, 63 | 64 (a wave border), 255 | 256 (a
         round border), 4095 | 4096 (a chunk border).
  d      255 / 256 / 257 records: site_rows_kernel runs n + 1 threads (256: one full block, 257 and 258: a second block of one and
         two), join_rows_kernel n threads (255, 256: one block, 257: a second block of one); budgets 1 and 0: two one-word launches.
  classes (a1)  map of 4 x 49610 = 198440 entries = 49 chunks, segment_bounds_kernel and join_pick_kernel before each join."""
import ctypes as C
import functools

import numpy as np
import pytest

import offtarget_cases as cases
import offtarget_ref as R
import panel_ref
from multiprime_amd.validate import amplicons

A_ROWS = [0, 3, 11, 12, 13, 10]                 # the sequences of case a1 in the order of the report (the issue's list)


@functools.lru_cache(maxsize=None)
def reduced(name):
    c = cases.get(name)
    return R.sites_of(c.seqs, c.reads, c.budgets, c.term)


@functools.lru_cache(maxsize=None)
def model(name):
    c = cases.get(name)
    return R.screen_of(reduced(name), c.primer, c.lo, c.hi)


def rows_of(products):
    return list(dict.fromkeys(p[0] for p in products))


def both_rows(name):
    """[(row, forward, reverse)] of the rows with sites on both strands."""
    c = cases.get(name)
    _, winners, _ = reduced(name)
    f, r = R.by_row(winners, 0, c.primer), R.by_row(winners, 1, c.primer)
    return [(row, f[row], r[row]) for row in sorted(set(f) & set(r))]


def store_offsets(seqs):
    return np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)


def map_indices(name, strand):
    c = cases.get(name)
    off = store_offsets(c.seqs)
    return {int(off[row]) + p for (s, row, p) in reduced(name)[1] if s == strand}


def encode_store(seqs):
    return np.frombuffer("".join(seqs).encode(), np.uint8), store_offsets(seqs)


def tuples(a):
    return [tuple(x) for x in a.tolist()]


# ---- CPU: the model is the checker ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_model_hits_equal_the_checkers_scan(oracle_lib, name):
    c = cases.get(name)
    per_read = reduced(name)[0]
    ctx = oracle_lib.context(0)
    try:
        ctx.seq_load(*encode_store(c.seqs))
        for budget in sorted(set(c.budgets)):
            idx = [i for i, b in enumerate(c.budgets) if b == budget]
            got = tuples(ctx.kmm_scan_resident(*R.encode([c.reads[i] for i in idx]), budget, c.term))
            want = sorted((row, p, k, strand) for k, i in enumerate(idx) for row, p, strand in per_read[i])
            assert want and got == want, budget
    finally:
        ctx.close()


@pytest.mark.parametrize("name", cases.NAMES)
def test_model_join_equals_amplicons(name):
    c = cases.get(name)
    products, counts = model(name)
    rows = both_rows(name)
    assert rows and counts["forward_sites"] > 0 and counts["reverse_sites"] > 0
    total = 0
    for row, f, r in rows:
        want = amplicons(f, r, c.lo, c.hi)
        assert R.row_products(f, r, c.lo, c.hi) == want == panel_ref.join(f, r, c.lo, c.hi), row
        assert [p[1:] for p in products if p[0] == row] == want
        total += len(want)
    assert counts["products"] == len(products) == total
    assert (total == 0) == name.endswith("none")


# ---- CPU: the cases contain what they are built for (from the model alone) ------------------------------------------------------------
def test_case_a1_order_shared_sites_and_record_borders():
    c = cases.get("a1")
    per_read, winners, row_min = reduced("a1")
    products, counts = model("a1")
    assert rows_of(products) == A_ROWS and A_ROWS != sorted(A_ROWS)
    assert len(set(c.primer)) < len(c.primer) and c.primer != list(range(len(c.primer)))          # two reads per primer, no identity
    tables = {b: max(len(r) for r, rb in zip(c.reads, c.budgets) if rb == b) > 32 for b in set(c.budgets)}
    assert sorted(tables.values()) == [False, False, True, True]                                   # four launches, two per kernel form
    # sites claimed by reads of different budgets: across launches
    claimed = {}
    for i, hl in enumerate(per_read):
        for row, p, strand in hl:
            claimed.setdefault((strand, row, p), set()).add(c.budgets[i])
    shared = [s for s, b in claimed.items() if len(b) > 1]
    assert len(shared) >= 10 and all(winners[s] == max(i for i, hl in enumerate(per_read) if (s[1], s[2], s[0]) in set(hl)) for s in shared[:10])
    assert any(len(b) >= 3 and s[0] == 1 for s, b in claimed.items())                              # RC(B): every S_m on one start
    # a row whose smallest read of ANY strand is smaller than its smallest forward read: row_min must not take reverse hits
    any_min = {}
    for i, hl in enumerate(per_read):
        for row, p, strand in hl:
            any_min.setdefault(row, i)
    assert any(any_min[row] < row_min[row] for row in row_min)
    assert R.row_order(row_min) != R.row_order({row: any_min[row] for row in row_min})
    # a forward site of one record and a reverse site of the next record with bases, as near in store offsets as a product
    off = store_offsets(c.seqs)
    f, r = R.by_row(winners, 0, c.primer), R.by_row(winners, 1, c.primer)
    with_bases = [row for row, s in enumerate(c.seqs) if s]
    crossing = 0
    for row, nxt in zip(with_bases, with_bases[1:]):
        a = np.array(sorted(f.get(row, ())), np.int64) + off[row]
        b = np.array(sorted(r.get(nxt, ())), np.int64) + off[nxt]
        n = b[None, :] - a[:, None] + 1
        crossing += int(((c.lo < n) & (n < c.hi)).sum())
    assert crossing > 0
    assert all(0 <= p[1] < p[2] < len(c.seqs[p[0]]) for p in products)
    assert counts["hits"] > counts["forward_sites"] + counts["reverse_sites"]                       # the map folds hits


def test_case_a1_reversed_reads_change_winners_and_order():
    a, b = cases.get("a1"), cases.get("a1rev")
    assert a.reads == b.reads[::-1] and a.budgets == b.budgets[::-1] and a.seqs == b.seqs
    n = len(a.reads)
    wa, wb = reduced("a1")[1], reduced("a1rev")[1]
    assert set(wa) == set(wb)                                                                       # the same sites ...
    assert any(wa[s] != n - 1 - wb[s] for s in wa)                                                  # ... of other reads
    pa, pb = model("a1")[0], model("a1rev")[0]
    assert pa != pb and len(pb) > 0
    assert rows_of(pa) != rows_of(pb) and sorted(rows_of(pa)) == sorted(rows_of(pb))


def test_case_a2_dead_starts_cut_products():
    c = cases.get("a2")
    cut = []
    for row, f, r in both_rows("a2"):
        starts, stops = sorted(f), sorted(r)
        rejected = stops[0] - starts[-1] > c.hi or stops[-1] - starts[0] < c.lo
        if not rejected and len(R.row_products(f, r, c.lo, c.hi)) < len(R.plain_filter(f, r, c.lo, c.hi)):
            cut.append(row)
    assert len(cut) >= 4, cut
    assert model("a2")[1]["products"] > 0


def test_case_a3_whole_row_rejects():
    c = cases.get("a3")
    rejected = []
    for row, f, r in both_rows("a3"):
        starts, stops = sorted(f), sorted(r)
        if stops[0] - starts[-1] > c.hi or stops[-1] - starts[0] < c.lo:
            rejected.append(row)
            assert R.row_products(f, r, c.lo, c.hi) == []
    assert len(rejected) >= 3, rejected
    assert model("a3")[1]["products"] > 0


def test_case_b_full_map_and_winners_by_length():
    c = cases.get("b")
    lengths = [len(r) for r in c.reads]
    assert lengths == sorted(lengths) and [len(s) for s in c.seqs] == [8193, 33]
    _, winners, _ = reduced("b")
    products, counts = model("b")
    legal = sum(len(s) - lengths[0] + 1 for s in c.seqs)
    assert counts["forward_sites"] == counts["reverse_sites"] == legal and legal % 256 != 0 and -(-legal // 2048) == 5
    assert counts["products"] > 0 and counts["both_genes"] == 2
    for strand in (0, 1):
        for row, s in enumerate(c.seqs):
            for p in range(len(s) - lengths[0] + 1):
                # the largest index that HITS there: the longest read that still fits (of two of one length the later)
                assert winners[(strand, row, p)] == max(i for i, n in enumerate(lengths) if p + n <= len(s)), (strand, row, p)
            tail = [winners[(strand, row, p)] for p in range(max(0, len(s) - 70), len(s) - lengths[0] + 1)]
            # towards the record's end the winner steps down, once per read length that fits the record
            assert tail == sorted(tail, reverse=True) and len(set(tail)) == len({n for n in lengths if n <= len(s)}) >= 4 and tail[-1] == 0


@pytest.mark.parametrize("total", [8191, 8192, 8193])
def test_case_c_sites_on_the_maps_borders(total):
    name = f"c{total}"
    c, forward, reverse = cases.case_c(total)
    assert c == cases.get(name) and sum(map(len, c.seqs)) == total
    assert [len(s) == 0 for s in c.seqs] == [True, False, True, False, False, True, False, True]
    assert 0 < min(len(s) for s in c.seqs if s) < min(map(len, c.reads))                            # a record shorter than every read
    assert map_indices(name, 0) == forward and map_indices(name, 1) == reverse                      # the model finds the plants, no more
    assert cases.c_required(total) <= forward
    off = store_offsets(c.seqs)
    inner = cases.C_INNER
    assert {int(off[inner]), int(off[inner + 1]) - 4, total - 4} <= forward
    assert {o + cases.C_STEP for o in forward if o != total - 4} == reverse
    assert c.lo < cases.C_STEP + 1 < c.hi
    # the reverse half of the map starts inside a chunk, on a chunk border, one past it
    assert (total % 4096, -(-2 * total // 4096)) == {8191: (4095, 4), 8192: (0, 4), 8193: (1, 5)}[total]
    products, counts = model(name)
    assert counts["products"] > 0 and rows_of(products) == [1, 3, 6]
    # the forward site at the end of the inner record has its partner's distance in a later record: no product
    assert not any(int(off[p[0]]) + p[1] == int(off[inner + 1]) - 4 for p in products)
    assert {p[3] for p in products} == {p[4] for p in products} == set(c.primer)                    # both reads win somewhere


def test_case_c_without_products():
    products, counts = model("c8192none")
    assert products == [] and counts["products"] == 0
    assert counts["forward_sites"] > 0 and counts["reverse_sites"] > 0 and counts["both_genes"] == 3


@pytest.mark.parametrize("n", [255, 256, 257])
def test_case_d_many_short_records(n):
    c = cases.get(f"d{n}")
    assert len(c.seqs) == n and max(map(len, c.seqs)) <= 40
    assert n // 5 <= sum(1 for s in c.seqs if not s) <= n // 3
    products, counts = model(c.name)
    rows = rows_of(products)
    assert n // 5 <= len(rows) <= n // 2 and rows != sorted(rows)
    assert n - 1 in rows                                                                            # the last record gives a product
    assert len(set(c.budgets)) == 2


def test_class_model_with_one_class_is_the_plain_screen():
    c = cases.get("a1")
    got, counts = R.screen_classes(c.seqs, c.reads, c.primer, [1] * len(c.reads), c.budgets, c.term, c.lo, c.hi)
    products, plain = model("a1")
    assert got == [p + (2,) for p in sorted(products, key=lambda p: p[0])] and counts == plain
    mixed, _ = R.screen_classes(c.seqs, c.reads, c.primer, cases.A_CLASSES, c.budgets, c.term, c.lo, c.hi)
    assert {p[6] for p in mixed} == {0, 1, 2}


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def args_of(c):
    return (*R.encode(c.reads), np.array(c.primer, np.int32), np.array(c.budgets, np.int32))


def raw_call(lib, ctx, c, cap, hi=None):
    """One mp_offtarget_resident as it is: (return code, *n_out, the buffer of max(cap, 1) products that went in filled with -1)."""
    codes, poff, primer, mm = args_of(c)
    out = np.full((max(cap, 1), 6), -1, np.int32)
    n = C.c_int64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = lib.dll.mp_offtarget_resident(ctx.h, len(c.reads), p(codes), p(poff), p(primer), p(mm), c.term, c.lo, c.hi if hi is None else hi, cap,
                                       p(out), C.byref(n))
    return rc, n.value, out


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.NAMES)
def test_screen_equals_model(hip_lib, name):
    c = cases.get(name)
    want, want_counts = model(name)
    ctx = hip_lib.context(0)
    try:
        ctx.seq_load(*encode_store(c.seqs))
        got = tuples(ctx.offtarget_resident(*args_of(c), c.term, c.lo, c.hi))
        counts = ctx.offtarget_stats()[1]
    finally:
        ctx.close()
    assert counts == want_counts
    assert len(got) == len(want) and rows_of(got) == rows_of(want)
    assert got == want
    assert (len(want) == 0) == name.endswith("none")


@pytest.mark.gpu
def test_gap_entry_without_gaps_equals_model(hip_lib):
    ctx = hip_lib.context(0)
    try:
        ctx.seq_load(*encode_store(cases.get("a1").seqs))
        for name in ("a1", "a2", "a3"):
            c = cases.get(name)
            codes, poff, primer, mm = args_of(c)
            got = tuples(ctx.offtarget_gap_resident(codes, poff, primer, 6 * mm + 3, 0, c.term, c.lo, c.hi))
            want, want_counts = model(name)
            assert len(want) > 0 and got == want, name
            assert ctx.offtarget_stats()[1] == want_counts, name
    finally:
        ctx.close()


@pytest.mark.gpu
def test_class_screen_equals_model(hip_lib):
    c = cases.get("a1")
    codes, poff, primer, mm = args_of(c)
    products, plain_counts = model("a1")
    ctx = hip_lib.context(0)
    try:
        ctx.seq_load(*encode_store(c.seqs))
        for classes in (cases.A_CLASSES, (1,) * len(c.reads)):
            got = tuples(ctx.offtarget_classes(codes, poff, primer, np.array(classes, np.int32), mm, c.term, c.lo, c.hi))
            want, want_counts = R.screen_classes(c.seqs, c.reads, c.primer, classes, c.budgets, c.term, c.lo, c.hi)
            assert len(want) > 0 and got == want, classes
            assert ctx.offtarget_stats()[1] == want_counts, classes
        # (the last pass: every read new) the plain screen's products, rows ascending, all of the join new x new
        assert got == [p + (2,) for p in sorted(products, key=lambda p: p[0])] and want_counts == plain_counts
    finally:
        ctx.close()


NOWHERE = "ACGTTGCATGCATCGATCGATTAGCACGTTGCA"     # 32 bases that no store of the cases holds: at budget 0 a call without a site


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a1", "b", "d257"])
def test_device_bytes_balance(hip_lib, name):
    """mp_device_bytes around every entry that drives the store scan.  What a call leaves on the device is a function of that call
    alone: the store, plus the products an off-target screen keeps for its repeat (a call without a site keeps an empty list of one
    slot).  So the reading after a call is the same every time that call is the last one made, in whatever order the calls ran —
    for the entries that keep nothing on the device it is the store's; and the two calls that touch no kept state at all (the
    validation scan, and a call refused for its arguments before anything is dropped) leave the reading exactly as they found it,
    which is the form the statement takes for them: what an earlier screen kept is still there and still counted."""
    c = cases.get(name)
    codes, poff, primer, mm = args_of(c)
    classes = np.arange(len(c.reads), dtype=np.int32) % 2
    none = R.encode([NOWHERE])
    short = R.encode(["ACG"])
    one = np.zeros(1, np.int32)
    sites = np.array([[0, 0, 5, 1], [0, 2, 7, 1], [1, 0, 40, 2], [1, 2, 90, 2]], np.int32)
    csites = np.array([[0, 0, 0, 5, 1], [0, 1, 0, 60, 2], [1, 0, 0, 9, 3], [1, 1, 0, 40, 4], [1, 1, 3, 40, 4]], np.int32)
    ctx = hip_lib.context(0)

    def refused():
        with pytest.raises(Exception, match="pattern 0 has length 3"):
            ctx.offtarget_resident(*short, one, one, c.term, c.lo, c.hi)

    def no_site():
        assert len(ctx.offtarget_resident(*none, one, one * 0, c.term, c.lo, c.hi)) == 0
        counts = ctx.offtarget_stats()[1]
        assert counts["forward_sites"] == counts["reverse_sites"] == 0

    calls = {
        "offtarget_resident": lambda: ctx.offtarget_resident(codes, poff, primer, mm, c.term, c.lo, c.hi),
        "offtarget_gap_resident": lambda: ctx.offtarget_gap_resident(codes, poff, primer, 6 * mm + 8, 1, c.term, c.lo, c.hi),
        "offtarget_classes": lambda: ctx.offtarget_classes(codes, poff, primer, classes, mm, c.term, c.lo, c.hi),
        "amplicon_join": lambda: ctx.amplicon_join(sites, 20, 100),
        "amplicon_join_classes": lambda: ctx.amplicon_join_classes(csites, 20, 100),
        "kmm_scan_resident": lambda: ctx.kmm_scan_resident(codes, poff, int(max(c.budgets)), c.term),
        "zero_patterns": lambda: ctx.offtarget_resident(np.zeros(1, np.uint8), np.zeros(1, np.int32), one[:0], one[:0], c.term, c.lo, c.hi),
        "no_site": no_site,
        "refused": refused,
    }
    untouched = {"kmm_scan_resident", "refused"}                     # no kept state read or written
    store_only = {"offtarget_classes", "amplicon_join", "amplicon_join_classes", "zero_patterns"}
    order = list(calls)
    rng = np.random.default_rng(5)
    # every call after every other one at least once: the list, its reverse, each call twice in a row (the repeat is served from
    # what the first kept), and two shuffles
    runs = [order, order[::-1], [n for n in order for _ in (0, 1)], list(rng.permutation(order)), list(rng.permutation(order))]
    seen = {n: set() for n in calls}
    try:
        before = ctx.device_bytes()
        ctx.seq_load(*encode_store(c.seqs))
        store = ctx.device_bytes()
        assert store - before == ctx.seq_info()[2] > 0
        last = store
        for run in runs:
            for n in run:
                calls[n]()
                now = ctx.device_bytes()
                if n in untouched:
                    assert now == last, (n, now, last)
                else:
                    seen[n].add(now)
                last = now
        assert all(len(seen[n]) == 1 for n in calls if n not in untouched), seen
        assert all(seen[n] == {store} for n in store_only), (seen, store)
        assert seen["no_site"] == {store + 6 * 4}                     # the empty list's one slot
        assert min(seen["offtarget_resident"]) > store and min(seen["offtarget_gap_resident"]) > store     # products are kept
        ctx.seq_free()
        assert ctx.device_bytes() == before
    finally:
        ctx.close()


@pytest.mark.gpu
def test_device_bytes_balance_of_the_set_screen(hip_lib, monkeypatch):
    """begin -> adds -> end returns to the reading before begin, with a list of one record of headroom and a pair table of one slot:
    both are regrown during the adds."""
    monkeypatch.setenv("MP_SETSCREEN_SITES", "1")
    monkeypatch.setenv("MP_SETSCREEN_TABLE", "1")
    c = cases.get("a1")
    reads = sorted(c.reads, key=len)                                  # the 4-base read and the palindrome first: sites everywhere
    ctx = hip_lib.context(0)
    try:
        before = ctx.device_bytes()
        ctx.seq_load(*encode_store(c.seqs))
        store = ctx.device_bytes()
        for _ in (0, 1):
            ctx.setscreen_begin(c.lo, c.hi, 1, 0)
            regrows = np.zeros(2, np.int64)
            for first in (0, 2, 4):
                batch = reads[first:first + 2]
                ctx.setscreen_add(*R.encode(batch), np.arange(first, first + len(batch), dtype=np.int32))
                counts = ctx.setscreen_stats()[1]
                regrows += (counts["list_regrows"], counts["table_regrows"])
            assert (regrows > 0).all(), regrows
            assert ctx.device_bytes() > store
            ctx.setscreen_end()
            assert ctx.device_bytes() == store
        ctx.setscreen_begin(c.lo, c.hi, 1, 0)                          # the store goes under an open screen: its device side goes too
        ctx.setscreen_add(*R.encode(reads[:2]), np.arange(2, dtype=np.int32))
        ctx.seq_free()
        assert ctx.device_bytes() == before
        ctx.setscreen_end()
        assert ctx.device_bytes() == before
    finally:
        ctx.close()


@pytest.mark.gpu
def test_kept_products(hip_lib):
    a, b = cases.get("a1"), cases.get("b")
    want, want_counts = model("a1")
    wider = R.screen_of(reduced("a1"), a.primer, a.lo, a.hi + 1)[0]
    on_b = R.screen(b.seqs, a.reads, a.primer, a.budgets, a.term, a.lo, a.hi)[0]
    assert len(want) > 0 and len(on_b) > 0 and len(wider) > 0
    ctx = hip_lib.context(0)
    scan_ms = lambda: ctx.offtarget_stats()[0]["scan_ms"]      # noqa: E731
    try:
        ctx.seq_load(*encode_store(a.seqs))
        rc, n, out = raw_call(hip_lib, ctx, a, 0)                                  # cap 0: the whole count, nothing written
        assert rc == 0 and n == len(want) and (out == -1).all() and scan_ms() > 0
        rc, n, out = raw_call(hip_lib, ctx, a, len(want))                          # the exact size: the kept list, no scan
        assert rc == 0 and n == len(want) and tuples(out) == want and scan_ms() == 0
        assert ctx.offtarget_stats()[1] == want_counts                             # the counts of the call that made them
        rc, n, out = raw_call(hip_lib, ctx, a, len(wider), hi=a.hi + 1)            # another range: scanned again
        assert rc == 0 and n == len(wider) and tuples(out) == wider and scan_ms() > 0
        rc, n, out = raw_call(hip_lib, ctx, a, len(want))
        assert rc == 0 and tuples(out) == want and scan_ms() > 0
        assert raw_call(hip_lib, ctx, a, len(want))[1] == len(want) and scan_ms() == 0
        joined = ctx.amplicon_join(np.array([[0, 0, 5, 1], [1, 0, 40, 2]], np.int32), 20, 100)      # explicit sites drop what was kept
        assert tuples(joined) == [(0, 5, 40, 1, 2, 36)]
        rc, n, out = raw_call(hip_lib, ctx, a, len(want))
        assert rc == 0 and tuples(out) == want and scan_ms() > 0
        ctx.seq_load(*encode_store(b.seqs))                                        # another store: the same arguments, its products
        rc, n, out = raw_call(hip_lib, ctx, a, len(on_b))
        assert rc == 0 and n == len(on_b) and tuples(out) == on_b and scan_ms() > 0
    finally:
        ctx.close()
