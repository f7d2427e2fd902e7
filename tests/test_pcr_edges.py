"""The exact in-silico PCR scan where pcr_block_kernel<NW, RES> and pcr_kernel<LONG> change behaviour (tests/pcr_cases.py plants the
sites): the 4096-position segment border and its over-packed tail words, the 3072-entry occurrence list and its per-pair fall-back,
the 4096-entry pattern table and the call that rolls as a whole, 32 / 33 bases, the 8-base prefix filter, a site cut by a record's
end, the reverse site that must end inside the Product, the non-overlapping next forward copy, the expansion order, case and N.

CPU leg: the checker's byte scan and its scan of the store against pcr_cases.model (the reference script's own expression on str),
and the outcome of every planted situation literally.  GPU leg (`-m gpu`): the HIP byte scan and the HIP scan of the resident store
against the checker, again with MP_PCR_ROLLING=1, again with MP_PCR_NO_PREFILTER=1 where the filter is on, and after a second load
of a prefix of the records."""
import numpy as np
import pytest

import pcr_cases as pc

_MODEL, _CHECKER = {}, {}


def _model(call):
    if call.name not in _MODEL:
        _MODEL[call.name] = pc.model(call.records, call.primers)
    return _MODEL[call.name]


def _tuples(a):
    return [[tuple(t) for t in rows] for rows in a.tolist()]


def _scans(lib, call, records=None):
    """(byte scan, scan of the store) of one call, one context."""
    data, off = pc.encode(call.records if records is None else records)
    codes, poff = pc.encode_primers(call.primers)
    ctx = lib.context(0)
    try:
        by_bytes = _tuples(ctx.pcr_scan(data, off, codes, poff))
        ctx.seq_load(data, off)
        return by_bytes, _tuples(ctx.pcr_scan_resident(codes, poff))
    finally:
        ctx.close()


def _checker(oracle_lib, call):
    if call.name not in _CHECKER:
        _CHECKER[call.name] = _scans(oracle_lib, call)
    return _CHECKER[call.name]


def _check_situations(call, got):
    for situation, pair, r, res in call.expect:
        assert got[call.pair(pair)][r] == res, (call.name, situation, pair, r)


@pytest.mark.parametrize("group", pc.GROUP_NAMES)
def test_every_situation_is_what_it_claims(group):
    """By the model alone: every planted situation gives the outcome written next to it, the occurrence counts are exact, no pattern
    stands outside the planted spans, and the calls have the shapes the kernels' limits ask for."""
    calls = pc.calls(group)
    for call in calls:
        assert pc.unplanted(call) == [], call.name
        _check_situations(call, _model(call))
        assert call.expect and all(len(rows) == len(call.records) for rows in _model(call))
        for r, n in call.counts:
            assert pc.occurrences(call.records[r], pc.patterns_of(call.primers)) == n, (call.name, r)
        lengths = {len(p) for pr in call.primers for p in pr}
        assert (min(lengths) >= 8) == (group in pc.FILTERED), call.name
    names = [c.name.split("/")[1] for c in calls]
    if group == "G_table":
        assert [pc.table_size(c) for c in calls] == [pc.TABLE, pc.TABLE + 2, pc.TABLE + 1] * 2
        assert calls[0].records is calls[5].records and len(calls[0].records) <= 20 and max(map(len, calls[0].records)) <= 600
        assert [{len(p) for pr in c.primers for p in pr} for c in calls] == [{20}] * 3 + [{40}] * 3
        hits = {e[3][0] for c in calls for e in c.expect}
        assert {1024, 2047, 2048, 4095} <= hits and {2046, 2047} <= {e[3][2] for c in calls for e in c.expect}
        return
    spec = pc.GROUPS[group]
    assert names == ["main", "single", "tiny257"] + (["occurrences"] if group in pc.OCC_GROUPS else [])
    main, single, tiny = calls[:3]
    assert len(single.records) == 1 and len(tiny.records) == 257 and max(map(len, tiny.records)) <= 2 * 64
    assert {e[1] for e in tiny.expect if e[2] == 256 and e[3] != pc.NONE} == {"main"}       # the row of the second block has a hit
    lengths = {len(p) for pr in main.primers for p in pr}
    assert lengths == {n for key in ("main", "selfov", "dege") for n in spec[key]} | {spec["pal"]} | {n for e in spec["extras"] for n in e}
    assert (max(lengths) > 32) == (group in ("G_two", "G_64"))
    L = spec["main"][0]
    assert L == max(lengths) and pc.table_size(main) < pc.TABLE
    said = [e[0] for e in main.expect if e[1] != "main_dup"]
    for s in list(range(pc.SEG - L, pc.SEG + 1)) + [2 * pc.SEG - L, 2 * pc.SEG - 1, 2 * pc.SEG]:
        assert "forward site at %d" % s in said
    for prefix in ("reverse site straddles", "reverse site ends a record of 4095", "reverse site ends a record of 4096",
                   "reverse site ends a record of 4097", "forward site at the last legal start", "record ends with half of F",
                   "record begins with the other half of F", "record ends with half of a palindromic F", "record ends with half of RC(R)",
                   "record one base shorter", "one-base record", "empty record first", "empty record in the middle", "empty record last",
                   "(a)", "(b)", "(c)", "(d)", "(e)", "(f)", "(g)", "(h) lower", "(h) N", "(h) R", "(h) lower-case product", "(j)"):
        assert any(s.startswith(prefix) for s in said), prefix
    assert main.records[0] == "" and main.records[-1] == "" and "" in main.records[1:-1]
    assert {pc.SEG - 1, pc.SEG, pc.SEG + 1} <= set(map(len, main.records))
    # (i) the pair listed twice answers twice, hits among the answers
    m = _model(main)
    assert main.primers[main.pair("main_dup")] == main.primers[main.pair("main")] and m[main.pair("main_dup")] == m[main.pair("main")]
    assert sum(t != pc.NONE for t in m[main.pair("main")]) > L
    # (j) two entries of the table are the same pattern, twice
    pats = pc.patterns_of(main.primers[:-1])
    assert len(pats) - len(set(pats)) >= 2
    if group in pc.OCC_GROUPS:
        assert sorted(n for _, n in calls[3].counts) == sorted(pc.OCC_COUNTS + (pc.HITS, pc.HITS + 1))
        assert len(calls[3].primers) == 1 and len(calls[3].primers[0][0]) == pc.OCC_GROUPS[group][0]


@pytest.mark.parametrize("group", pc.GROUP_NAMES)
def test_checker_equals_the_model(oracle_lib, group):
    for call in pc.calls(group):
        by_bytes, by_store = _checker(oracle_lib, call)
        assert by_bytes == _model(call), call.name
        assert by_store == _model(call), call.name
        _check_situations(call, by_bytes)


def _hip_equals_checker(hip_lib, oracle_lib, unit):
    for call in pc.unit_calls(unit):
        want = _checker(oracle_lib, call)[0]
        assert want == _checker(oracle_lib, call)[1]
        by_bytes, by_store = _scans(hip_lib, call)
        assert by_bytes == want, call.name + ": byte scan"
        assert by_store == want, call.name + ": resident scan"
        _check_situations(call, by_bytes)
        _check_situations(call, by_store)


@pytest.mark.gpu
@pytest.mark.parametrize("unit", pc.UNITS, ids=pc.UNIT_IDS)
def test_hip_scans_equal_the_checker(hip_lib, oracle_lib, unit, monkeypatch):
    import torch  # noqa: F401
    monkeypatch.delenv("MP_PCR_ROLLING", raising=False)
    monkeypatch.delenv("MP_PCR_NO_PREFILTER", raising=False)
    _hip_equals_checker(hip_lib, oracle_lib, unit)


@pytest.mark.gpu
@pytest.mark.parametrize("unit", pc.UNITS, ids=pc.UNIT_IDS)
def test_hip_rolling_scans_equal_the_checker(hip_lib, oracle_lib, unit, monkeypatch):
    import torch  # noqa: F401
    monkeypatch.setenv("MP_PCR_ROLLING", "1")
    monkeypatch.delenv("MP_PCR_NO_PREFILTER", raising=False)
    _hip_equals_checker(hip_lib, oracle_lib, unit)


@pytest.mark.gpu
@pytest.mark.parametrize("unit", [u for u in pc.UNITS if u[0] in pc.FILTERED], ids=[i for u, i in zip(pc.UNITS, pc.UNIT_IDS) if u[0] in pc.FILTERED])
def test_hip_scans_without_the_prefix_filter_equal_the_checker(hip_lib, oracle_lib, unit, monkeypatch):
    import torch  # noqa: F401
    monkeypatch.delenv("MP_PCR_ROLLING", raising=False)
    monkeypatch.setenv("MP_PCR_NO_PREFILTER", "1")
    _hip_equals_checker(hip_lib, oracle_lib, unit)


@pytest.mark.gpu
@pytest.mark.parametrize("group", pc.GROUP_NAMES)
def test_hip_resident_scan_after_a_second_load_of_a_prefix(hip_lib, oracle_lib, group, monkeypatch):
    """The second load replaces the store: the scan sees the prefix alone (its last record spans the segment border)."""
    import torch  # noqa: F401
    monkeypatch.delenv("MP_PCR_ROLLING", raising=False)
    monkeypatch.delenv("MP_PCR_NO_PREFILTER", raising=False)
    call = pc.calls(group)[0]
    n = min(12, len(call.records) // 2 + 1)
    data, off = pc.encode(call.records)
    pdata, poff_rows = pc.encode(call.records[:n])
    codes, poff = pc.encode_primers(call.primers)
    h = hip_lib.context(0)
    try:
        h.seq_load(data, off)
        h.seq_load(pdata, poff_rows)
        assert h.seq_info()[:2] == (n, len(pdata))
        got = _tuples(h.pcr_scan_resident(codes, poff))
    finally:
        h.close()
    want = [rows[:n] for rows in _checker(oracle_lib, call)[0]]
    assert got == want
    assert any(t != pc.NONE for rows in want for t in rows)
    assert np.array_equal(poff_rows, off[:n + 1])
