"""The set screen on the device (csrc/setscreen.hip, include/mprime_setscreen.h) against the model of the rule in
tests/setscreen_ref.py: the join alone on explicit sites, scan + join through begin / add, and get_Maxprimerset -r end to end on
the recorded fixture.  Every case first checks that the model's answer is not empty."""
import contextlib
import io
import os
import types

import numpy as np
import pytest

import setscreen_cases as cases
import setscreen_ref as ref
from conftest import GOLDEN
from multiprime_amd import iupac, maxset
from multiprime_amd._abi import SETSCREEN_BIN, MprimeError

pytestmark = pytest.mark.gpu
FIX = os.path.join(GOLDEN, "setscreen")
P31 = (1 << 31) - 1


# ---- the join alone ----------------------------------------------------------------------------------------------------------------------
def model_join(sites, lo, hi):
    """the double loop of the rule over explicit (strand, row, pos, primer) sites -> sorted (A, B, count)"""
    fwd = [s for s in sites if s[0] == 0]
    rev = [s for s in sites if s[0] == 1]
    table = {}
    for _, ra, pa, a in fwd:
        for _, rb, pb, b in rev:
            if ra == rb and lo < pb - pa + 1 < hi:
                table[(a, b)] = table.get((a, b), 0) + 1
    return sorted((a, b, n) for (a, b), n in table.items())


def dev_join(ctx, sites, lo, hi, **kw):
    s = np.array(sorted(set(sites)), np.int32).reshape(-1, 4)
    return [tuple(t) for t in ctx.setscreen_join(s, lo, hi, **kw).tolist()]


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.context(0)
    yield c
    c.close()


LO, HI = 150, 400
JOIN_CASES = {
    # lengths exactly lo, lo + 1, hi - 1, hi (one reverse primer each): only the middle two count
    "bounds": ([(0, 0, 100, 0)] + [(1, 0, 100 + n - 1, 1 + i) for i, n in enumerate((LO, LO + 1, HI - 1, HI))], LO, HI),
    # the end of row 0 and the start of row 1 are six store offsets apart: no product; the pair inside row 0 counts
    "row_border": ([(0, 0, 980, 0), (1, 0, 990, 1), (1, 1, 5, 2), (0, 1, 50, 3)], 0, 100),
    "same_position": ([(0, 3, 50, 0), (1, 3, 50, 1)], 0, 3),
    "two_primers_one_site": ([(0, 0, 10, 0), (0, 0, 10, 1), (1, 0, 200, 2), (1, 0, 200, 3)], LO, HI),
    "forward_only_and_self": ([(0, 0, 10, 0), (0, 0, 20, 1), (1, 0, 220, 1), (0, 2, 7, 0)], LO, HI),
    "far": ([(0, 70000, P31 - 500, 0), (1, 70000, P31, 1), (1, 70000, P31 - 1, 2), (0, 65536, 3, 3), (1, 65536, 203, 3)], LO, 502),
}


@pytest.mark.parametrize("name", sorted(JOIN_CASES))
def test_join_on_explicit_sites(ctx, name):
    sites, lo, hi = JOIN_CASES[name]
    want = model_join(sites, lo, hi)
    assert want
    assert dev_join(ctx, sites, lo, hi) == want
    if name == "bounds":
        assert want == [(0, 2, 1), (0, 3, 1)]
    if name == "row_border":
        assert want == [(0, 1, 1)]


def test_join_of_no_site_and_of_one(ctx):
    assert model_join(JOIN_CASES["same_position"][0], 0, 3) and dev_join(ctx, JOIN_CASES["same_position"][0], 0, 3) == [(0, 1, 1)]
    assert dev_join(ctx, [], LO, HI) == [] and dev_join(ctx, [(0, 0, 5, 0)], LO, HI) == [] and dev_join(ctx, [(1, 0, 5, 0)], LO, HI) == []


@pytest.mark.parametrize("span", [100, SETSCREEN_BIN, 3000])
def test_join_across_bin_borders(ctx, span):
    """a start just below a bin border, stops on both sides of it and of the next borders; hi - lo below, at and above the bin width"""
    lo, hi = 10, 10 + span
    start = SETSCREEN_BIN - 24
    at = [9, 10, 23, 24, 30, 100, 109, 110, SETSCREEN_BIN - 1, SETSCREEN_BIN, SETSCREEN_BIN + 9, SETSCREEN_BIN + 10, 2 * SETSCREEN_BIN - 1,
          2 * SETSCREEN_BIN, 3000, 3008, 3009, 3010]
    sites = [(0, 0, start, 0), (0, 0, start + SETSCREEN_BIN, 1)] + [(1, 0, start + k, 2 + (i % 3)) for i, k in enumerate(at)]
    want = model_join(sites, lo, hi)
    assert want
    assert dev_join(ctx, sites, lo, hi) == want


def test_join_of_random_sites_with_a_table_of_one_slot(ctx, monkeypatch):
    rng = np.random.default_rng(5)
    sites = sorted({(int(rng.integers(0, 2)), int(rng.integers(0, 3)), int(rng.integers(0, 5000)), int(rng.integers(0, 9))) for _ in range(700)})
    want = model_join(sites, LO, HI)
    assert len(want) > 40
    assert dev_join(ctx, sites, LO, HI, cap=3) == want              # (a small cap: the second call)
    monkeypatch.setenv("MP_SETSCREEN_TABLE", "1")
    assert dev_join(ctx, sites, LO, HI) == want
    assert ctx.setscreen_stats()[1]["table_regrows"] > 0


# ---- scan + join -----------------------------------------------------------------------------------------------------------------------------
def encode(reads_per_primer, first):
    flat = [r for rs in reads_per_primer for r in rs]
    codes = iupac.MASK_LUT[np.frombuffer("".join(flat).encode(), np.uint8)]
    off = np.zeros(len(flat) + 1, np.int32)
    np.cumsum([len(r) for r in flat], out=off[1:])
    rp = np.repeat(np.arange(first, first + len(reads_per_primer), dtype=np.int32), [len(rs) for rs in reads_per_primer])
    return codes, off, rp


def load(ctx, rows):
    data = np.frombuffer("".join(rows).encode(), np.uint8)
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(s) for s in rows], out=off[1:])
    ctx.seq_load(data, off)


def screen(ctx, rows, primers, dist, m, lo, hi, batch=None):
    """(sorted triples over all adds, forward site counts, reverse site counts, the stats of every add)"""
    load(ctx, rows)
    ctx.setscreen_begin(lo, hi, m, ref.TERM_MATCH)
    try:
        out, stats = [], []
        step = batch or len(primers)
        for i in range(0, len(primers), step):
            out += [tuple(t) for t in ctx.setscreen_add(*encode([ref.reads_of(p, dist) for p in primers[i:i + step]], i)).tolist()]
            stats.append(ctx.setscreen_stats())
        f, r = ctx.setscreen_site_counts(0, len(primers))
        return sorted(out), f.tolist(), r.tolist(), stats
    finally:
        ctx.setscreen_end()


@pytest.fixture(scope="module")
def planted():
    """One record of 20 000 bases and two short ones; dist 0 (whole primers), m = 1, 150 < length < 2000."""
    rng = np.random.default_rng(23)
    rows = [cases.rnd(rng, 20000), cases.rnd(rng, 700), cases.rnd(rng, 40)]
    mk = lambda n: cases.rnd(rng, n)                                       # noqa: E731
    deg = "ACGTRCCGATTC"                                                    # both expansions hit one place at m = 1
    cases.plant(rows, 0, 300, "ACGTACCGATTC")
    r_deg = mk(14)
    cases.plant_reverse(rows, 0, 700, r_deg, 0)
    f_seg, r_seg, f_edge = mk(16), mk(16), mk(12)                           # around the 8192-start segment border
    cases.plant_forward(rows, 0, 8100, f_seg, 0)
    cases.plant_reverse(rows, 0, 8300, r_seg, 0)
    cases.plant_forward(rows, 0, 8186, f_edge, 0)
    long_f, long_r = mk(40), mk(45)                                         # the two-word kernel
    cases.plant_forward(rows, 0, 12000, long_f, 0)
    cases.plant_reverse(rows, 0, 12900, long_r, 0)
    cases.plant_forward(rows, 0, 16370, long_f, 0)                          # a long read across the second segment border
    cases.plant_reverse(rows, 0, 16700, long_r, 0)
    pal = "AACGTTAACGTT"                                                    # its own reverse complement
    cases.plant(rows, 1, 100, pal)
    cases.plant(rows, 1, 400, pal)
    f_low, r_n = mk(15), mk(15)                                             # lower case counts, an N is a mismatch
    cases.plant(rows, 0, 5000, f_low.lower())
    site = list(cases.rc(r_n))
    site[3] = "N"
    cases.plant(rows, 0, 5400, "".join(site))
    cases.plant(rows, 0, 5600, "".join(site[:3]) + "NN" + "".join(site[5:]))     # two mismatches: no site at m = 1
    nowhere = "ACGTTGCATGCATCGATCGATTAGC"
    primers = [deg, r_deg, f_seg, r_seg, f_edge, long_f, long_r, pal, f_low, r_n, nowhere]
    site_map = ref.sites(rows, primers, 0, 1)
    table = ref.pair_table(site_map, 150, 2000)
    ids = {p: i for i, p in enumerate(primers)}
    return rows, primers, site_map, ref.triples(table, ids), ids


def test_scan_and_join_equal_the_model(ctx, planted):
    rows, primers, site_map, want, ids = planted
    assert len(want) >= 5
    got, f, r, stats = screen(ctx, rows, primers, 0, 1, 150, 2000)
    assert got == want
    assert f == [len(site_map[p][0]) for p in primers] and r == [len(site_map[p][1]) for p in primers]
    # what the planted cases are about
    assert f[ids["ACGTRCCGATTC"]] == 1                                       # two reads, one site
    assert (ids[primers[2]], ids[primers[3]], 1) in want                     # joined across the segment border
    assert (ids[primers[5]], ids[primers[6]], 2) in want                     # reads of more than 32 bases
    assert (ids["AACGTTAACGTT"], ids["AACGTTAACGTT"], 1) in want             # the palindrome pairs with itself
    assert (ids[primers[8]], ids[primers[9]], 1) in want                     # lower case, and one N within the budget
    assert f[-1] == 0 and r[-1] == 0                                         # a primer with no site at all
    assert stats[0][1]["scan_launches"] == 2 and stats[0][1]["pairs"] == len(want)


def test_adds_one_by_one_equal_one_add(ctx, planted):
    rows, primers, _, want, _ = planted
    assert want
    got, _, _, stats = screen(ctx, rows, primers, 0, 1, 150, 2000, batch=1)
    assert got == want and stats[-1][1]["adds"] == len(primers)


def test_small_list_and_table_regrow_to_the_same_result(ctx, planted, monkeypatch):
    rows, primers, site_map, want, _ = planted
    assert want
    monkeypatch.setenv("MP_SETSCREEN_SITES", "1")
    monkeypatch.setenv("MP_SETSCREEN_TABLE", "1")
    got, f, _, stats = screen(ctx, rows, primers, 0, 1, 150, 2000, batch=4)
    assert got == want and f == [len(site_map[p][0]) for p in primers]
    assert sum(s[1]["list_regrows"] for s in stats) > 0 and sum(s[1]["table_regrows"] for s in stats) > 0


def test_cap_zero_and_one_are_served_from_the_kept_result(ctx, planted):
    rows, primers, _, want, _ = planted
    assert len(want) > 1
    args = encode([ref.reads_of(p, 0) for p in primers], 0)
    load(ctx, rows)
    ctx.setscreen_begin(150, 2000, 1, ref.TERM_MATCH)
    try:
        for cap in (0, 1):
            part, n = ctx.setscreen_add_raw(*args, cap)
            assert n == len(want) and len(part) == cap
            ms, counts = ctx.setscreen_stats()
            if cap:                                                          # the repeat scanned nothing
                assert counts["scan_launches"] == 0 and ms["scan_ms"] == 0 and ms["join_ms"] == 0
                assert tuple(part[0].tolist()) in want
            else:
                assert counts["scan_launches"] > 0
        full, n = ctx.setscreen_add_raw(*args, len(want))
        assert sorted(tuple(t) for t in full.tolist()) == want and ctx.setscreen_stats()[1]["scan_launches"] == 0
    finally:
        ctx.setscreen_end()


def test_one_hot_pair_from_many_workgroups(ctx):
    """20 000 bases of a 10-mer: every tenth position is a site of F and of R; one (F, R) count fed by every workgroup"""
    unit = "ACGGTCATGC"
    rows = [unit * 2000]
    f, r = (unit * 2)[:12], cases.rc((unit * 2)[3:15])
    lo, hi = 150, 400
    site_map = ref.sites([rows[0][:200]], [f, r], 0, 0)                     # the model on a slice: the phase of the sites
    assert sorted(site_map[f][0]) == [(0, p) for p in range(0, 181, 10)] and sorted(site_map[r][1]) == [(0, p) for p in range(3, 184, 10)]
    assert not site_map[f][1] and not site_map[r][0]
    starts, stops = np.arange(0, 20000 - 11, 10), np.arange(3, 20000 - 11, 10)
    # closed form: per start the stops with lo <= stop - start <= hi - 2
    want = int(sum(np.searchsorted(stops, s + hi - 2, "right") - np.searchsorted(stops, s + lo, "left") for s in starts))
    assert want > 40000
    got, nf, nr, _ = screen(ctx, rows, [f, r], 0, 0, lo, hi)
    assert nf == [len(starts), 0] and nr == [0, len(stops)]
    assert got == [(0, 1, want)]


def test_call_order_errors_are_codes(ctx, planted):
    rows = planted[0]
    args = encode([["ACGTACGTACGT"]], 0)
    with pytest.raises(MprimeError) as e:                                    # add before begin
        ctx.setscreen_add(*args)
    assert e.value.code == -1
    load(ctx, rows[1:])
    ctx.setscreen_begin(150, 2000, 1, 5)
    try:
        with pytest.raises(MprimeError) as e:                                # begin twice
            ctx.setscreen_begin(150, 2000, 1, 5)
        assert e.value.code == -1
        ctx.setscreen_add(*args)
        load(ctx, rows[2:])                                                  # the store replaced under a live screen
        with pytest.raises(MprimeError) as e:
            ctx.setscreen_add(*encode([["ACGTACGTACGA"]], 1))
        assert e.value.code == -1 and "store" in str(e.value)
    finally:
        ctx.setscreen_end()
    ctx.setscreen_begin(150, 2000, 1, 5)                                     # and a fresh screen works
    assert ctx.setscreen_add(*args).shape == (0, 3)
    ctx.setscreen_end()


# ---- the script --------------------------------------------------------------------------------------------------------------------------------
def run_script(lib, tmp_path, sub, extra):
    d = tmp_path / sub
    d.mkdir()
    inp, out = d / "candidates.txt", d / "final.xls"
    inp.write_text(open(os.path.join(FIX, "candidates.txt")).read())
    opts = maxset.parse_args(["-i", str(inp), "-o", str(out)] + extra)
    with contextlib.redirect_stdout(io.StringIO()):
        maxset.run(opts, library=lib)
    return {p.name: p.read_text() for p in d.iterdir()}


def test_script_with_and_without_a_background(hip_lib, tmp_path):
    recorded = {n: open(os.path.join(FIX, n)).read() for n in os.listdir(FIX)}
    assert "rejected" in recorded["final.xls.offtarget.tsv"] and "selected" in recorded["final.xls.offtarget.tsv"]
    for sub, extra in (("k4", []), ("k1", ["--lookahead", "1"]), ("k1000", ["--lookahead", "1000"])):
        got = run_script(hip_lib, tmp_path, sub, ["-r", os.path.join(FIX, "background.fa")] + extra)
        for name in ("final.xls", "final.xls.offtarget.tsv", "final.xls.offtarget.set.tsv", "fina.next.xls"):
            assert got[name] == recorded[name], (sub, name)
    plain = run_script(hip_lib, tmp_path, "plain", [])
    assert sorted(plain) == ["candidates.txt", "fina.next.xls", "final.xls", "sort.candidates.txt"]
    assert plain["final.xls"] == recorded["plain.final.xls"] and plain["fina.next.xls"] == recorded["plain.fina.next.xls"]
