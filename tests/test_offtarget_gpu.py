"""The off-target screen on the device (include/mprime_offtarget.h, csrc/offtarget.hip) against its checker, the host path of
validate.py: mp_amplicon_join against validate.amplicons() on seeded site sets (the quirk cases, products past the caller's cap),
and mp_offtarget_resident through the drop-in of scripts/primer_specificity.py against validate's scan sites through amplicons() and
the same report code — byte-identical files on a background of 3 x 10^7 bases with more than 2^20 hits."""
import ctypes as C

import numpy as np
import pytest

from multiprime_amd.specificity import off_targets
from multiprime_amd.synth import offtarget_case
from multiprime_amd.validate import amplicons


def _expected(forward, reverse, lo, hi):
    """Rows ascending, validate.amplicons() per row with sites on both strands."""
    out = []
    for row in sorted(forward):
        if row in reverse:
            out.extend((row,) + p for p in amplicons(forward[row], reverse[row], lo, hi))
    return out


def _sites(forward, reverse):
    s = [(0, r, p, f[p]) for r, f in forward.items() for p in f] + [(1, r, p, v[p]) for r, v in reverse.items() for p in v]
    return np.array(sorted(s), np.int32).reshape(-1, 4)


def _random_sites(rng, n_rows, density, row_len):
    forward, reverse = {}, {}
    for row in range(n_rows):
        for d in (forward, reverse):
            n = int(rng.poisson(density))
            if n:
                d[row] = {int(p): int(rng.integers(0, 7)) for p in rng.integers(0, row_len, size=n)}
    return forward, reverse


def _join(ctx, forward, reverse, lo, hi, cap):
    got = ctx.amplicon_join(_sites(forward, reverse), lo, hi, cap=cap)
    return [tuple(x) for x in got.tolist()]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_join_equals_amplicons_on_random_sites(seed, hip_lib):
    rng = np.random.default_rng(700 + seed)
    lo, hi = [(100, 1500), (50, 400), (20, 60), (0, 3000), (100, 1500), (300, 320)][seed]
    forward, reverse = _random_sites(rng, 60, [3, 40, 200, 25, 400, 80][seed], [5000, 20000, 4000, 30000, 100000, 8000][seed])
    want = _expected(forward, reverse, lo, hi)
    ctx = hip_lib.context(0)
    try:
        assert _join(ctx, forward, reverse, lo, hi, cap=1 << 20) == want
        assert _join(ctx, forward, reverse, lo, hi, cap=7) == want          # past the cap: the count, then the retry with the exact size
        assert ctx.offtarget_stats()[1]["products"] == len(want)
    finally:
        ctx.close()
    assert seed == 0 or len(want) > 7


@pytest.mark.gpu
def test_join_quirks(hip_lib):
    f = {100: 1, 120: 2, 5000: 3, 5100: 4}
    r = {400: 11, 1599: 12, 1600: 13, 5300: 14}
    f2 = dict(f)
    f2[3000] = 5                                   # no stop in range: 5000 and 5100 are never looked at
    forward = {0: f, 1: f2, 2: {10: 1}, 3: {10: 1}, 4: {10: 1, 20: 2}, 6: {7: 1}, 7: {100: 1, 101: 2, 102: 3}}
    reverse = {0: r, 1: r, 2: {5000: 9}, 3: {50: 9}, 5: {300: 9}, 6: {300: 9},
               7: {199: 9, 200: 8, 1599: 7, 1600: 6, 1601: 5}}    # row 7: lengths size_lo - 1 .. + 1 and size_hi - 1 .. + 1
    want = _expected(forward, reverse, 100, 1500)
    ctx = hip_lib.context(0)
    try:
        got = _join(ctx, forward, reverse, 100, 1500, cap=1000)
        # the raw call with a short buffer: *n_out is the whole count, the buffer holds the first `cap` products in order
        sites = _sites(forward, reverse)
        buf = np.zeros((3, 6), np.int32)
        n = C.c_int64(0)
        rc = hip_lib.dll.mp_amplicon_join(ctx.h, len(sites), sites.ctypes.data_as(C.c_void_p), 100, 1500, 3, buf.ctypes.data_as(C.c_void_p), C.byref(n))
        with pytest.raises(Exception, match="ascend"):
            ctx.amplicon_join(sites[::-1].copy(), 100, 1500)
    finally:
        ctx.close()
    assert got == want
    assert rc == 0 and n.value == len(want) and [tuple(x) for x in buf.tolist()] == want[:3]
    assert {row for row, *_ in want} == {0, 1, 6, 7}
    assert [p[1] for p in want if p[0] == 1] == [100, 120, 120, 120]                      # the dead start 3000 ends row 1
    lengths = {p[5] for p in want if p[0] == 7}
    assert {101, 1499} <= lengths and not lengths & {100, 1500}


def _run_both(tmp_path, hip_lib, pf, bf, **kw):
    outs = {}
    for join in ("device", "host"):
        out = tmp_path / f"{join}.out"
        app = off_targets(primer_file=pf, reference_file=bf, outfile=str(out), library=hip_lib, join=join, **kw)
        app.run()
        outs[join] = (app, [(tmp_path / (f"{join}.out" + s)).read_bytes() for s in ("", ".pair.num", ".total.acc.num")])
    return outs


@pytest.mark.gpu
def test_resident_screen_equals_host_path_past_the_hit_cap(tmp_path, hip_lib, capsys):
    """3 x 10^7 bases, 384 reads of 9 bases (12 primers with N, N, R in the term) with one mismatch allowed outside the 4-base 3'
    term: more than 2^20 hits — the host path's scan overflows its 2^20-hit buffer and scans again, the device path has no hit
    buffer at all.  (bowtie2's own budget for 9 bases is 0 mismatches: --max-mismatch 1 makes the hits.)"""
    pf, bf = offtarget_case(str(tmp_path / "in"), 300, 100_000, 12, 1)
    outs = _run_both(tmp_path, hip_lib, pf, bf, term_length=9, PCR_product_size="100,400", term_threshold=4, max_mismatch=1)
    dev, host = outs["device"], outs["host"]
    assert dev[1] == host[1]
    st = dev[0].stats
    assert st["hits"] > 1 << 20 and st["products"] > 10000, st
    assert host[1][0].count(b"\n") == st["products"] + 1
    capsys.readouterr()


@pytest.mark.gpu
def test_resident_screen_mixed_budgets_and_long_reads(tmp_path, hip_lib, capsys):
    """Whole primers as reads (term length 0): 20-base reads (budget 2), a 40-base one (the two-word kernel, budget 4) and a
    12-base one (budget 1) — one launch per budget — on a small background; then the --max-mismatch override; then a repeat with a
    tiny cap, served from the products the library kept."""
    rng = np.random.default_rng(5)
    pf, bf = offtarget_case(str(tmp_path / "in"), 40, 20_000, 6, 2, n_degenerate=1)
    bg = open(bf).read().split("\n")
    seq0 = bg[1]
    long_read = seq0[3000:3040]
    short_read = "".join("ACGT"[i] for i in rng.integers(0, 4, size=12))
    rc = seq0[5000:5020].translate(str.maketrans("ACGT", "TGCA"))[::-1]
    with open(pf, "a") as f:
        f.write(f">L\n{long_read}\n>S\n{short_read}\n>T\n{seq0[4000:4012]}\n>RV\n{rc}\n")
    for kw in ({}, {"max_mismatch": 1}):
        outs = _run_both(tmp_path, hip_lib, pf, bf, term_length=0, PCR_product_size="30,3000", term_threshold=2, **kw)
        assert outs["device"][1] == outs["host"][1]
        assert outs["device"][0].stats["products"] > 0
    # the same call twice: the second with a cap below the count is answered from the kept products, without a scan
    from multiprime_amd import iupac
    from multiprime_amd.host import Fasta
    data, off = Fasta(bf).rows()
    reads = [long_read, seq0[4000:4012], rc, seq0[6000:6020]]        # forward 3000, 4000, 6000; reverse 5000
    codes = iupac.MASK_LUT[np.frombuffer("".join(reads).encode(), np.uint8)]
    poff = np.cumsum([0] + [len(r) for r in reads]).astype(np.int32)
    ctx = hip_lib.context(0)
    try:
        ctx.seq_load(data, off)
        budget = np.array([2, 0, 2, 2], np.int32)                    # the 12-base read exact: with 2 mismatches it hits at random
        full = ctx.offtarget_resident(codes, poff, np.arange(4, dtype=np.int32), budget, 2, 30, 3000)
        first, _ = ctx.offtarget_stats()
        again = ctx.offtarget_resident(codes, poff, np.arange(4, dtype=np.int32), budget, 2, 30, 3000, cap=1)
        second, counts = ctx.offtarget_stats()
    finally:
        ctx.close()
    assert [tuple(x) for x in full.tolist()] == [(0, 3000, 5000, 0, 2, 2001), (0, 4000, 5000, 1, 2, 1001)]
    assert again.tolist() == full.tolist()
    assert first["scan_ms"] > 0 and second["scan_ms"] == 0 and counts["products"] == len(full)
    capsys.readouterr()


def _rc(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


def _planted_case(tmp_path):
    """Four sequences of 20 kb, two primers with one R each, 12-base terms (bowtie2's budget: 1 mismatch).  Sequence 0: the sites
    offtarget_case plants (exact, one mismatch, a mismatch inside the 3' term; reverse partners 200-202 bases on).  Sequence 1: the
    second primer forward at 500, the first one's reverse complement at 700; sequence 2 the other way round.  So sequence 2's
    smallest forward read (0) is smaller than sequence 1's (2): the report lists sequence 2 before sequence 1.  A last record repeats
    sequence 1's name: the FASTA parser appends it to sequence 1, on both paths."""
    pf, bf = offtarget_case(str(tmp_path / "in"), 4, 20_000, 2, 3, n_degenerate=0, plant_len=12)
    primers = open(pf).read().split("\n")[1::2][:2]
    terms = [p[-12:].replace("R", "A") for p in primers]
    lines = open(bf).read().split("\n")

    def put(seq, at, site):
        return seq[:at] + site + seq[at + len(site):]
    lines[3] = put(put(lines[3], 500, terms[1]), 700, _rc(terms[0]))
    lines[5] = put(put(lines[5], 500, terms[0]), 700, _rc(terms[1]))
    rng = np.random.default_rng(9)
    lines[-1:] = [">bg000001 repeated name", "".join("ACGT"[i] for i in rng.integers(0, 4, size=3000)), ""]
    open(bf, "w").write("\n".join(lines))
    return pf, bf


def _check_planted(out_text):
    rows = [line.split("\t") for line in out_text.splitlines()[1:]]
    assert list(dict.fromkeys(r[0] for r in rows)) == ["bg000000", "bg000002", "bg000001"]      # (smallest forward read, row)
    seq0 = {(r[1], r[2]) for r in rows if r[0] == "bg000000"}
    assert ("100", "300") in seq0 and ("600", "801") in seq0                    # exact and one-mismatch sites
    assert not any(r[1] == "1100" for r in rows if r[0] == "bg000000")         # the mismatch inside the 3' term: no site
    assert ["bg000001", "500", "700", "P1", "P0", "201"] in rows and ["bg000002", "500", "700", "P0", "P1", "201"] in rows


@pytest.mark.gpu
def test_planted_sites_and_sequence_order(tmp_path, hip_lib, capsys):
    pf, bf = _planted_case(tmp_path)
    outs = _run_both(tmp_path, hip_lib, pf, bf, term_length=12, PCR_product_size="100,400", term_threshold=4)
    assert outs["device"][1] == outs["host"][1]
    _check_planted(outs["device"][1][0].decode())
    capsys.readouterr()
