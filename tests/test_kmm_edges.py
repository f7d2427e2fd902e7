"""The k-mismatch scan where kmm_kernel<NW, RES> changes behaviour (tests/kmm_cases.py plants the sites): the 8192-start segment
border and its overhang words, the 32-base word border of the packed store, the last legal start of a record, a site cut by a
record's end, records shorter than a pattern, counted mismatches and trailing match runs, lower case, N, both strands, a palindrome,
term == len and term > len, the one-word and the two-word kernel.

CPU leg: the checker's byte scan and its resident scan against test_validate.brute (the rule of include/mprime.h, both strands in
text orientation).  GPU leg (`-m gpu`): the HIP byte scan and the HIP scan of the resident store against the checker's list, the
regrow path (cap 0 and 1), a second load of a prefix.  On both legs every planted tuple the rule admits must be in the result and
every one it rejects must be absent, so nothing passes on an empty list."""
import numpy as np
import pytest

import kmm_cases as kc
from test_validate import brute

CASES = ([(s, mm, term, None) for s in ("one", "two") for mm, term in kc.PARAMS] +
         [(f"eq{m}", 3, m, None) for m in kc.LENGTHS] +                # term == len on sets of equal-length patterns
         [(s, 64, 0, kc.CUT) for s in ("one", "two")])                 # every legal start of every pattern hits
IDS = [f"{s}-mm{mm}-term{term}" + ("-cut" if rows else "") for s, mm, term, rows in CASES]


def _inputs(set_name, rows):
    seqs, pats, _ = kc.database()
    first, end = rows or (0, len(seqs))
    names = kc.pattern_set(set_name)
    return list(seqs[first:end]), names, [pats[n] for n in names]


def _tuples(a):
    return [tuple(x) for x in a.tolist()]


def _scans(lib, seqs, strings, max_mm, term, caps=(None,)):
    """[byte scan, resident scan] per cap, as lists of tuples (the wrappers sort them)."""
    data, off = kc.encode(seqs)
    codes, poff = kc.encode_patterns(strings)
    ctx = lib.context(0)
    try:
        ctx.seq_load(data, off)
        out = []
        for cap in caps:
            kw = {} if cap is None else {"cap": cap}
            out.append((_tuples(ctx.kmm_scan(data, off, codes, poff, max_mm, term, **kw)), _tuples(ctx.kmm_scan_resident(codes, poff, max_mm, term, **kw))))
        return out
    finally:
        ctx.close()


def _check_plants(got, names, max_mm, term, rows):
    must, must_not, _ = kc.expected(names, max_mm, term, rows)
    got = set(got)
    assert must <= got, sorted(must - got)[:10]
    assert not must_not & got, sorted(must_not & got)[:10]
    return len(must), len(must_not)


_ORACLE = {}


def _oracle(oracle_lib, case):
    if case not in _ORACLE:
        s, mm, term, rows = case
        seqs, _, strings = _inputs(s, rows)
        _ORACLE[case] = _scans(oracle_lib, seqs, strings, mm, term)[0]
    return _ORACLE[case]


_BRUTE = {}


def _brute(case):
    """test_validate.brute on the case.  It decides every pattern by itself, so the list of the one-word set on the whole database is
    the list of the two-word set (which holds the same patterns and more) cut to those patterns: computed once, shared."""
    s, mm, term, rows = case
    seqs, names, strings = _inputs(s, rows)
    if s != "one" or rows:
        if case not in _BRUTE:
            _BRUTE[case] = brute(seqs, strings, mm, term)
        return _BRUTE[case]
    wide = kc.pattern_set("two")
    index = {wide.index(n): i for i, n in enumerate(names)}
    return sorted((r, p, index[i], strand) for r, p, i, strand in _brute(("two", mm, term, rows)) if i in index)


def test_builder_plants_every_category():
    """The database is what the module says, and over the cases below every category has tuples that must hit and tuples that must
    not (a cut site and a too-short record have no legal start: only tuples that must not)."""
    seqs, pats, plants = kc.database()
    assert tuple(len(s) for s in seqs) == kc.RECORD_LENGTHS and len(seqs) == 14 and sum(map(len, seqs)) < 51000
    assert {len(p) for p in pats.values()} == set(kc.LENGTHS) and pats["PAL"] == kc.rc(pats["PAL"])
    assert max(len(pats[n]) for n in kc.pattern_set("one")) == 32 and max(len(pats[n]) for n in kc.pattern_set("two")) == 64
    total = {c: [0, 0] for c in kc.CATEGORIES}
    for s, mm, term, rows in CASES:
        must, must_not, by = kc.expected(kc.pattern_set(s), mm, term, rows)
        for c in kc.CATEGORIES:
            total[c][0] += by[c][0]
            total[c][1] += by[c][1]
        if term > 64:
            assert not must and must_not
        elif mm == 64:                            # only a start without room for the pattern is rejected
            assert must and all(t in kc.expected(kc.pattern_set(s), 0, 0, rows)[1] for t in must_not)
        else:
            assert must and must_not
    for c in kc.CATEGORIES:
        assert total[c][1] > 0 and (total[c][0] > 0) == (c not in kc.NEVER_HIT), (c, total[c])
    # the starts the issue names, for every pattern length
    at = {(p["cat"], p["r"], p["start"], p["pat"]) for p in plants}
    for m in kc.LENGTHS:
        assert {("segment", 11, kc.SEG - m, f"S{m}"), ("segment", 3, kc.SEG - m + 1, f"S{m}"), ("segment", 12, kc.SEG - 1, f"S{m}"),
                ("segment", 13, kc.SEG, f"S{m}"), ("word", 0, 0, f"S{m}"), ("word", 10, 31, f"S{m}"), ("word", 11, 32, f"S{m}"),
                ("word", 3, 33, f"S{m}"), ("last", 2, 65 - m, f"S{m}"), ("cut", 8, 63 - (m - 1), f"S{m}")} <= at


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_checker_scans_equal_brute_force(oracle_lib, case):
    s, mm, term, rows = case
    seqs, names, strings = _inputs(s, rows)
    want = _brute(case)
    by_bytes, by_store = _oracle(oracle_lib, case)
    assert by_bytes == want
    assert by_store == want
    n_must, n_not = _check_plants(want, names, mm, term, rows)
    assert (n_not > 0 or mm == 64) and (n_must > 0 or term > 64)
    if mm == 64:                                  # nothing but the end of the record rejects a start
        assert len(want) == sum(2 * max(0, len(q) - len(p) + 1) for q in seqs for p in strings)
    if term > 64:
        assert want == []


def test_store_of_empty_records(oracle_lib):
    """Context.seq_load hands a text of no bytes over as a valid pointer: records that are all empty make a store, not a refusal."""
    codes, poff = kc.encode_patterns(["ACGT"])
    ctx = oracle_lib.context(0)
    try:
        ctx.seq_load(np.zeros(0, np.uint8), np.zeros(4, np.int64))
        assert ctx.seq_info()[:2] == (3, 0)
        assert ctx.kmm_scan_resident(codes, poff, 1, 0).shape == (0, 4)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hip_scans_equal_the_checker(hip_lib, oracle_lib, case):
    import torch  # noqa: F401
    s, mm, term, rows = case
    seqs, names, strings = _inputs(s, rows)
    want = _oracle(oracle_lib, case)[0]
    assert want == _oracle(oracle_lib, case)[1]
    default, cap0, cap1 = _scans(hip_lib, seqs, strings, mm, term, caps=(None, 0, 1))
    assert default[0] == want, "byte scan"
    assert default[1] == want, "resident scan"
    _check_plants(default[0], names, mm, term, rows)
    _check_plants(default[1], names, mm, term, rows)
    assert cap0 == default and cap1 == default    # the count of a first pass sizes the second


@pytest.mark.gpu
@pytest.mark.parametrize("set_name", ["one", "two"])
def test_hip_resident_scan_after_a_second_load_of_a_prefix(hip_lib, oracle_lib, set_name):
    import torch  # noqa: F401
    seqs, names, strings = _inputs(set_name, None)
    codes, poff = kc.encode_patterns(strings)
    data, off = kc.encode(seqs)
    pdata, poff_rows = kc.encode(seqs[:kc.PREFIX])
    h, o = hip_lib.context(0), oracle_lib.context(0)
    try:
        h.seq_load(data, off)
        h.seq_load(pdata, poff_rows)
        assert h.seq_info()[:2] == (kc.PREFIX, len(pdata))
        for mm, term in ((1, 4), (2, 0)):
            want = _tuples(o.kmm_scan(pdata, poff_rows, codes, poff, mm, term))
            assert _tuples(h.kmm_scan_resident(codes, poff, mm, term)) == want
            must, must_not, _ = kc.expected(names, mm, term, (0, kc.PREFIX))
            assert must and must <= set(want) and not must_not & set(want)
    finally:
        h.close()
        o.close()


@pytest.mark.gpu
def test_hip_store_of_empty_records(hip_lib):
    import torch  # noqa: F401
    codes, poff = kc.encode_patterns(["ACGT"])
    ctx = hip_lib.context(0)
    try:
        ctx.seq_load(np.zeros(0, np.uint8), np.zeros(4, np.int64))
        assert ctx.seq_info()[:2] == (3, 0)
        assert ctx.kmm_scan_resident(codes, poff, 1, 0).shape == (0, 4)
    finally:
        ctx.close()
