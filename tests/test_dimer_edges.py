"""The 3'-end dimer scan kernels of multiprime_amd/csrc/dimer.hip (dimer_group_kernel<16|64>, dimer_rows_kernel<32|64-bit planes>,
dimer_pairs_kernel<32|64-bit planes>, the split walk of mp_dimer_pairs, the staged / global Loss table, the host's choice of form) at their
edges, against tests/dimer_ref.py: the rule on strings.  The CPU tests pin that model to the oracle record for record and assert that the
cases of tests/dimer_cases.py contain what they are built for; the GPU tests compare the kernels with the model (small sets) or with
the oracle (sets too large for Python)."""
import ctypes as C
import gzip
import os
import random
from itertools import product

import numpy as np
import pytest

import dimer_cases as cases
import dimer_ref as R
from conftest import GOLDEN
from multiprime_amd.dimer import cached_loss_table, dg_limit, dg_params, encode_primers

THRESHOLDS = [3.96, 3.0, -20.0, 60.0]      # finDimer's, get_Maxprimerset's, below every Loss (any match passes), above every Loss (deltaG alone)
LANES = ["1", "16", "64", None]


def tables(threshold):
    return cached_loss_table(threshold), dg_params(), dg_limit()


def scan(ctx, seqs, mode, n_new, threshold, cap=1 << 16):
    codes, off = encode_primers(seqs)
    return [tuple(r) for r in ctx.dimer_scan(codes, off, mode, n_new, *tables(threshold), cap=cap).tolist()]


def flags(ctx, seqs, pairs, threshold):
    codes, off = encode_primers(seqs)
    return ctx.dimer_pairs(codes, off, np.array(pairs, np.int32).reshape(-1, 2), *tables(threshold)).tolist()


def small_sets():
    """name -> (primers, n_new values): every set the Python model walks all against all."""
    out = {}
    for name, seqs in (("ladder", cases.length_ladder(False)), ("ladder_long", cases.length_ladder(True)),
                       ("boundary", cases.boundary_set()[0]), ("degenerate", cases.degenerate_light()[0])):
        out[name] = (seqs, [0, 1, len(seqs) - 1, len(seqs)])
    heavy, n_new, _ = cases.degenerate_heavy()
    out["degenerate_heavy"] = (heavy, [n_new])
    return out


SMALL = ["ladder", "ladder_long", "boundary", "degenerate", "degenerate_heavy"]


def modes_of(name):
    return (1,) if name == "degenerate_heavy" else (0, 1)


def d2_of(seqs, rec):
    x, y, l, ei, pi, idx = rec
    return len(seqs[y]) - l - idx


def end_of(seqs, rec):
    x, y, l, ei, pi, idx = rec
    return R.expand(seqs[x][-l:])[ei]


@pytest.fixture(scope="module")
def ora(oracle_lib):
    c = oracle_lib.context(0)
    yield c
    c.close()


# ---- CPU: the model is the oracle ------------------------------------------------------------------------------------------------------
def all_pairs_of(name, seqs, n_news):
    if name == "degenerate_heavy":
        return R.scan_pairs(len(seqs), 1, n_news[0])
    return [(x, y) for x in range(len(seqs)) for y in range(len(seqs))]


def check_against_model(ctx, name, threshold, **kw):
    """Both scan modes (mode 1 with every n_new of the set) and the pair list of every ordered pair: records equal to the model's."""
    seqs, n_news = small_sets()[name]
    for mode in modes_of(name):
        for n_new in (n_news if mode else n_news[:1]):
            assert scan(ctx, seqs, mode, n_new, threshold, **kw) == R.scan_records(seqs, mode, n_new, threshold), (mode, n_new)
    pairs = all_pairs_of(name, seqs, n_news)
    assert flags(ctx, seqs, pairs, threshold) == R.pair_flags(seqs, pairs, threshold)


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("name", SMALL)
def test_model_equals_oracle(ora, name, threshold):
    check_against_model(ora, name, threshold, cap=1 << 20)


@pytest.mark.parametrize("threshold", [3.96, 3.0])
def test_model_equals_oracle_on_a_golden_input(ora, threshold):
    """findimer_syn_a: the oracle's output on it is pinned to the unmodified reference by tests/test_dimer.py."""
    text = gzip.open(os.path.join(GOLDEN, "inputs", "findimer_syn_a.fa.gz")).read().decode()
    seqs = list(dict.fromkeys(line.strip() for line in text.splitlines() if line.strip() and not line.startswith(">")))
    want = R.scan_records(seqs, 0, 0, threshold)
    assert len(want) > 0 and scan(ora, seqs, 0, 0, threshold, cap=1 << 20) == want


# ---- CPU: the cases contain what they claim (from the model alone) ---------------------------------------------------------------------
def test_ladder_reaches_the_table_corners():
    short, long = cases.length_ladder(False), cases.length_ladder(True)
    assert {len(s) for s in short} >= set(cases.LENGTHS) and max(map(len, short)) == 32
    assert {len(s) for s in long} >= set(cases.LENGTHS + cases.LONG_LENGTHS) and max(map(len, long)) == 64
    for seqs in (short, long):
        low = R.scan_records(seqs, 0, 0, -20.0)
        assert {r[2] for r in low} >= {1, 2, 3, 4, 5, 6, 17, 18}                         # ends of 1..4 bases: primers shorter than 5
        assert any(len(seqs[r[1]]) < min(18, len(seqs[r[0]])) for r in low)              # a partner shorter than the longest end (ly < l)
        assert any(r[0] == r[1] and r[2] == 18 for r in low)                             # the palindrome with itself
        assert max(d2_of(seqs, r) for r in low) == max(map(len, seqs)) - 1               # a 1-base primer at the first base of the longest
        ms = R.scan_records(seqs, 1, len(seqs), 3.0)
        assert {r[2] for r in ms} >= {5, 16, 17, 18, 20, 21, 30, 31}                     # mode 1: more than 16 end lengths from 22 bases on
    assert max(d2_of(long, r) for r in R.scan_records(long, 0, 0, -20.0)) == 63
    ms = R.scan_records(long, 1, len(long), 3.0)
    assert {r[2] for r in ms} >= {32, 47, 62, 63}
    assert max(end_of(long, r).count("G") + end_of(long, r).count("C") for r in ms) >= 32


@pytest.mark.parametrize("name", SMALL)
def test_delta_g_alone_decides_above_every_loss(name):
    """At 60.0 no Loss passes (log10(2^128 / 0.01) < 41): every hit is flush and exactly the pairs hit whose first flush match is below -5."""
    seqs, n_news = small_sets()[name]
    for mode in modes_of(name):
        recs = R.scan_records(seqs, mode, n_news[-1], 60.0)
        assert recs and all(d2_of(seqs, r) == 0 and R.delta_g(end_of(seqs, r)) < -5 for r in recs)
        want = set()
        for x, y in R.scan_pairs(len(seqs), mode, n_news[-1]):
            if any(len(seqs[y]) - l - idx == 0 and R.delta_g(end) < -5 for l, ei, pi, idx, end in R.matches(seqs[x], seqs[y], mode)):
                want.add((x, y))
        assert {(r[0], r[1]) for r in recs} == want
        assert not any(R.pair_hit(seqs[x], seqs[y], mode, 60.0, with_delta_g=False) for x, y in want)


def test_boundary_ends_sit_on_the_rounding_boundary():
    found = cases.boundary_ends()
    assert set(found) >= {(-5.01, "plain"), (-5.01, "ta"), (-5.0, "plain"), (-5.0, "ta"), (-5.0, "sym"), (-4.99, "plain"), (-4.99, "ta")}
    assert "ACACTGTG" in found[(-5.0, "sym")] and not any(cls == "sym" for g, cls in found if g != -5.0)
    seqs, plan = cases.boundary_set()
    assert len(plan) >= 14
    for g, cls, x, flush, off in plan:
        for mode in (0, 1):
            hit = R.pair_hit(seqs[x], seqs[flush], mode, 60.0)
            assert (hit is not None) == (g == -5.01), (g, cls, seqs[x])
            assert hit is None or (seqs[x][-hit[0]:], len(seqs[flush]) - hit[0] - hit[3]) == (R.rc(seqs[flush])[:hit[0]], 0)
            assert R.pair_hit(seqs[x], seqs[off], mode, 60.0) is None


def test_no_shipped_threshold_needs_the_delta_g_clause():
    """At 3.96 and 3.0 Loss alone already reports every hit of the ladders, the boundary set and 2000 random pairs: a wrong deltaG
    changes nothing there, which is why the kernels are also run at 60.0."""
    rng = random.Random(4)
    prim = cases.random_primers(12, 400)
    sets = [(s, [(x, y) for x in range(len(s)) for y in range(len(s))]) for s in (cases.length_ladder(False), cases.boundary_set()[0])]
    sets.append((prim, [(rng.randrange(400), rng.randrange(400)) for _ in range(2000)]))
    for threshold in (3.96, 3.0):
        n = 0
        for seqs, pairs in sets:
            for x, y in pairs:
                for mode in (0, 1):
                    h = R.pair_hit(seqs[x], seqs[y], mode, threshold)
                    assert h == R.pair_hit(seqs[x], seqs[y], mode, threshold, with_delta_g=False)
                    n += h is not None
        assert n > 100
    # the arithmetic behind it: flush, Loss = log10(2^(l + GC) / 0.01) reaches 3.96 from l + GC = 7 and 3.0 for every end of 5 bases
    assert R.loss(5, 2, 0, 0) >= 3.96 > R.loss(5, 1, 0, 0) and R.loss(6, 0, 0, 0) < 3.96 and R.loss(5, 0, 0, 0) >= 3.0
    # and the ends Loss leaves out there (l + GC <= 6: five bases with at most one G/C, six with none) are nowhere near deltaG < -5
    weak = ["".join(e) for n, gc in ((5, 1), (6, 0)) for e in product("ACGT", repeat=n) if sum(c in "GC" for c in e) <= gc]
    assert len(weak) == 32 + 5 * 32 + 64 and min(R.delta_g(e) for e in weak) > -2


def test_degenerate_cases_contain_their_orders():
    seqs, named = cases.degenerate_light()
    assert max(len(R.expand(s)) for s in seqs) <= 48 and {len(R.MEMBERS[c]) for s in seqs for c in s} == {1, 2, 3, 4}
    x, y = named["first"]
    assert [m[:4] for m in R.matches(seqs[x], seqs[y], 0)][:2] == [(12, 0, 0, 12), (12, 1, 0, 0)]
    for threshold in THRESHOLDS:
        assert R.pair_hit(seqs[x], seqs[y], 0, threshold) == (12, 0, 0, 12)
    x, y = named["plain_partner"]
    assert R.pair_hit(seqs[x], seqs[y], 0, 3.96) == (18, 17, 0, 4)
    x, y = named["degenerate_partner"]
    l, ei, pi, idx = R.pair_hit(seqs[x], seqs[y], 0, 3.96)
    assert (l, idx) == (18, 3) and pi > 0
    heavy, n_new, named = cases.degenerate_heavy()
    x, y = named["last_end"]
    assert len(R.expand(heavy[x][-18:])) == 4096
    for mode in (0, 1):
        assert R.pair_hit(heavy[x], heavy[y], mode, 3.96) == (18, 4095, 0, 7)
    x, y = named["late_y"]
    assert len(R.expand(heavy[y])) == 4 * 3 ** 8
    assert R.pair_hit(heavy[x], heavy[y], 0, -20.0) == (9, 0, 4 * 3 ** 8 - 1, 0) and R.pair_hit(heavy[x], heavy[y], 0, 3.0) is None
    assert R.pair_hit(heavy[x], heavy[y], 1, -20.0) == (8, 0, 4 * (3 ** 8 - 1), 0)


@pytest.mark.parametrize("name", sorted(cases.DRAINS))
def test_drain_layouts_are_as_planned(name):
    plan = cases.DRAINS[name]
    seqs = cases.drain_set(plan)
    assert cases.drain_counts(seqs) == plan
    assert cases.STRIDE * (len(plan) - 1) < len(seqs) <= min(cases.STRIDE * len(plan), 1280)      # 1280: held512_then_511 needs five full strides
    survivors = [h + p for h, p in plan]
    queued, drains = 0, []
    for i, s in enumerate(survivors):                      # the queue as dimer_rows_kernel runs it: a drain at >= 256 waiting or on the last stride
        queued += s
        if queued >= 256 or i + 1 == len(survivors):
            drains.append(queued)
            queued = 0
    assert drains == {"q255_1": [256], "q256": [256], "q511": [511], "late300": [256, 44], "h512": [256, 256, 1], "h513": [256, 256, 2],
                      "h1023": [256, 256, 256, 256], "h1024": [256, 256, 256, 256, 1], "h1025": [256, 256, 256, 256, 2],
                      "held512_then_511": [256, 256, 256, 511], "passers600": [256, 256, 88]}[name]
    hits = {"h512": 512, "h513": 513, "h1023": 1023, "h1024": 1024, "h1025": 1025, "held512_then_511": 1023, "passers600": 0}
    assert name not in hits or sum(h for h, p in plan) == hits[name]
    if name == "held512_then_511":                         # records held when a drain ends: 512 is not flushed (512 + 512 fits), the next drain adds 511
        assert [sum(h for h, p in plan[:i]) for i in (1, 2, 3)] == [255, 511, 512] and sum(h for h, p in plan[3:]) == 511


def test_size_sets_straddle_the_host_thresholds():
    """The host counts n * n / 2 + n pairs for a mode-0 scan and takes 64 lanes per pair up to 32768, 16 up to 262144, else one thread.
    This DERIVES the form of each size set from that rule as read in dimer.hip (lanes_per_pair); it does not observe which kernel ran and
    would not notice a change of the rule there: it only keeps the sizes of dimer_cases on either side of the two switches as they stand."""
    for n, (visited, lanes) in cases.SCAN_SIZES.items():
        assert n * n // 2 + n == visited and lanes == (64 if visited <= 32768 else 16 if visited <= 262144 else 1)
    assert [cases.LIST_SIZES[p] for p in (32768, 32769, 262144, 262145)] == [64, 16, 16, 1]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.context(0)
    yield c
    c.close()


def set_lanes(monkeypatch, lanes):
    if lanes is None:
        monkeypatch.delenv("MP_DIMER_LANES", raising=False)
    else:
        monkeypatch.setenv("MP_DIMER_LANES", lanes)


# a list holding a primer of more than 32 bases takes the 64-bit-plane thread-per-pair kernels whatever MP_DIMER_LANES says: one run of it
FORMS = [(name, lanes) for name in SMALL for lanes in (["1"] if name == "ladder_long" else LANES)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,lanes", FORMS)
def test_kernels_equal_the_model(ctx, monkeypatch, name, lanes):
    """Both scan modes and the pair list of every ordered pair, four thresholds, every form."""
    set_lanes(monkeypatch, lanes)
    for threshold in THRESHOLDS:
        check_against_model(ctx, name, threshold)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", ["16", "64"])
@pytest.mark.parametrize("split", ["1", "2", "16", "64"])
def test_split_walk_of_the_pair_list(ctx, monkeypatch, split, lanes):
    """Several groups per pair OR their answers into a zeroed flag: pairs whose only passing combination lies far beyond the first
    split x G steps (expansion 4095 of the end, expansion 26 243 of the partner) beside pairs with one combination per end length."""
    monkeypatch.setenv("MP_DIMER_LANES", lanes)
    monkeypatch.setenv("MP_DIMER_SPLIT", split)
    for seqs, pairs in ((cases.degenerate_light()[0], None), (cases.degenerate_heavy()[0], R.scan_pairs(4, 1, 2))):
        pairs = pairs or [(x, y) for x in range(len(seqs)) for y in range(len(seqs))]
        for threshold in (3.96, -20.0, 60.0):
            want = R.pair_flags(seqs, pairs, threshold)
            assert 0 < sum(want) < len(want) and flags(ctx, seqs, pairs, threshold) == want, threshold


DRAIN_RUNS = [(name, mode, n_new) for name in sorted(cases.DRAINS) for mode, n_new in ((0, 0), (1, 256), (1, 257))]


@pytest.mark.gpu
@pytest.mark.parametrize("long", [False, True])
@pytest.mark.parametrize("name,mode,n_new", DRAIN_RUNS)
def test_queue_and_hit_buffer_boundaries(ctx, ora, hip_lib, monkeypatch, name, mode, n_new, long):
    """dimer_rows_kernel, both plane widths, mode 0 and mode 1 (a row at or beyond n_new ends at y1 = n_new: exactly one stride, and one
    stride plus one partner): rows whose filter survivors and hits sit on the queue's and the hit buffer's boundaries; then the raw call
    with a capacity at and below the count: *n_hits is the full count, the buffer holds min(cap, count) distinct records."""
    monkeypatch.setenv("MP_DIMER_LANES", "1")
    seqs = cases.drain_set(cases.DRAINS[name], long)
    threshold = 3.0 if mode else 3.96
    want = scan(ora, seqs, mode, n_new, threshold, cap=1 << 20)
    assert scan(ctx, seqs, mode, n_new, threshold) == want
    codes, off = encode_primers(seqs)
    loss, dg, limit = tables(threshold)
    count = len(want)
    assert count > 1
    for cap in (0, 1, count - 1, count):
        buf = np.full((max(cap, 1), 6), -1, np.int32)
        n = C.c_int64(-1)
        rc = hip_lib.dll.mp_dimer_scan(ctx.h, len(seqs), codes.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), mode, n_new,
                                       loss.ctypes.data_as(C.c_void_p), dg.ctypes.data_as(C.c_void_p), C.c_double(limit), C.c_int64(cap),
                                       buf.ctypes.data_as(C.c_void_p) if cap else None, C.byref(n))
        got = [tuple(r) for r in buf[:cap].tolist()]
        assert rc == 0 and n.value == count and len(set(got)) == cap and set(got) <= set(want), cap


@pytest.mark.gpu
@pytest.mark.parametrize("n", sorted(cases.SCAN_SIZES))
def test_default_form_across_the_scan_thresholds(ctx, ora, monkeypatch, n):
    """No MP_DIMER_LANES: 32767 pairs take 64 lanes per pair, 33024 and 262087 take 16, 262812 one thread per pair."""
    monkeypatch.delenv("MP_DIMER_LANES", raising=False)
    seqs = cases.random_primers(n, n)
    want = scan(ora, seqs, 0, 0, 3.96, cap=1 << 20)
    assert len(want) > n // 10 and scan(ctx, seqs, 0, 0, 3.96) == want


@pytest.mark.gpu
@pytest.mark.parametrize("n_pairs", sorted(cases.LIST_SIZES))
def test_default_form_across_the_pair_list_thresholds(ctx, ora, monkeypatch, n_pairs):
    monkeypatch.delenv("MP_DIMER_LANES", raising=False)
    monkeypatch.delenv("MP_DIMER_SPLIT", raising=False)
    seqs = cases.random_primers(300, 300)
    pairs = cases.pair_list(n_pairs, 300, n_pairs)
    want = flags(ora, seqs, pairs, 3.6)
    assert sum(want) > 50 and flags(ctx, seqs, pairs, 3.6) == want
