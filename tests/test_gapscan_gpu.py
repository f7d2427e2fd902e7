"""The gapped rule on the device (csrc/kmm.hpp: kmm_gap_kernel behind mp_kmm_gap_scan_resident and mp_offtarget_gap_resident) against
the brute-force enumerator of tests/test_gapscan.py: its planted and random cases (one pattern word at L <= 32, two at L = 40), starts
around the segment edges of a 17 kb row, the gapped off-target screen against validate.amplicons() fed with the brute-force sites,
both drop-in commands with --gaps, and the recorded bowtie2 run."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from multiprime_amd._abi import MprimeError
from multiprime_amd.validate import amplicons
from test_gapscan import (GBAR, LENGTHS, MAX_GAP, RANDOM_PEN, RANDOM_TERM, _bases, brute_min_gap, check_bowtie2_fixture_with_gaps, make_read,
                          pack_reads, pack_rows, planted_cases, planted_truth, random_case, random_truth, rc, site_text)

K_SEG = 8192            # start positions per workgroup of the scan


def _scan(ctx, rows, reads, pen, max_gap, term, **kw):
    ctx.seq_load(*pack_rows(rows))
    codes, off = pack_reads(reads)
    return [tuple(x) for x in ctx.kmm_gap_scan_resident(codes, off, pen, max_gap, term, **kw).tolist()]


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
def test_planted_sites_on_the_device(L, hip_lib):
    assert hip_lib.backend == "hip" and hip_lib.gapscan
    ctx = hip_lib.context(0)
    try:
        for (name, row, reads, pen, term, key, want), sites in zip(planted_cases(L), planted_truth(L)):
            assert (key in sites) == want, (L, name)
            got = _scan(ctx, [row], reads, pen, MAX_GAP, term)
            assert got == sites, (L, name)
            assert len(set(got)) == len(got), (L, name, "a site reported twice")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("words", (1, 2))
def test_random_database_on_the_device(words, hip_lib):
    """words = 1: the reads of up to 30 bases (one pattern word); 2: all twelve, the 40-base read with them (two words for the call)."""
    rows, reads = random_case()
    best = random_truth()
    n_reads = len(reads) if words == 2 else sum(1 for r in reads if len(r) <= 32)
    assert (max(len(r) for r in reads[:n_reads]) > 32) == (words == 2)
    ctx = hip_lib.context(0)
    try:
        for max_gap in range(MAX_GAP + 1):
            want = sorted(k for k, g in best.items() if g <= max_gap and k[2] < n_reads)
            assert _scan(ctx, rows, reads[:n_reads], RANDOM_PEN, max_gap, RANDOM_TERM) == want, max_gap
        # past a small cap: the count comes back, the wrapper asks again with the exact size
        assert _scan(ctx, rows, reads[:n_reads], RANDOM_PEN, MAX_GAP, RANDOM_TERM, cap=5) == want and len(want) > 5
        # max_gap = 0 is the ungapped scan
        codes, off = pack_reads(reads[:n_reads])
        assert ctx.kmm_gap_scan_resident(codes, off, RANDOM_PEN, 0, RANDOM_TERM).tolist() == \
            ctx.kmm_scan_resident(codes, off, RANDOM_PEN // 6, RANDOM_TERM).tolist()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_segment_edges(hip_lib):
    """Five rows of about 17,000 bases; row d carries type D sites (even d: the 18-base read, g = 2; odd d: the 40-base read, g = 1;
    rows 3 and 4 on the reverse strand) that START at 8188 + d and at 16380 + d — the last starts of a segment of 8192 and the first
    of the next, their windows reaching into the following segment's words — and one site that ends exactly at the row's end.  Row 0
    is 17,024 = 532 * 32 bases long: its last word is full."""
    short, long_ = make_read(18, seed=7), make_read(40, seed=8)
    rng = np.random.default_rng(99)
    rows, planted = [], []
    for d in range(5):
        read = (short, long_)[d % 2]
        site = site_text(read if d < 3 else rc(read), "D", 2 if d % 2 == 0 else 1, GBAR + 2 * d)
        n = 17024 if d == 0 else 17000 + d
        row = list(_bases(rng, n))
        for at in (K_SEG - 4 + d, 2 * K_SEG - 4 + d, n - len(site)):
            row[at:at + len(site)] = site
            planted.append((d, at, d % 2, 0 if d < 3 else 1))
        rows.append("".join(row))
    assert len(rows[0]) % 32 == 0
    reads = [short, long_]
    want = sorted(brute_min_gap(rows, reads, 11, 2))
    assert set(planted) <= set(want)
    ctx = hip_lib.context(0)
    try:
        assert _scan(ctx, rows, reads, 11, MAX_GAP, 2) == want                       # two pattern words
        assert _scan(ctx, rows, reads[:1], 11, MAX_GAP, 2) == [k for k in want if k[2] == 0]   # one
    finally:
        ctx.close()


def _expected_products(best, read_primer, max_gap, lo, hi):
    """mp_offtarget_resident's contract on brute-force sites: per (strand, row, position) the primer of the largest read that hits,
    rows in ascending (smallest read with a forward hit, row), validate.amplicons() per row."""
    sites = ({}, {})
    first = {}
    for (row, p, read, strand), g in sorted(best.items(), key=lambda kv: kv[0][2]):
        if g <= max_gap:
            sites[strand].setdefault(row, {})[p] = read_primer[read]
            if strand == 0:
                first.setdefault(row, read)
    out = []
    for row in sorted(first, key=lambda r: (first[r], r)):
        if row in sites[1]:
            out.extend((row,) + p for p in amplicons(sites[0][row], sites[1][row], lo, hi))
    return out


@pytest.mark.gpu
def test_gapped_screen_equals_amplicons_of_brute_force_sites(hip_lib):
    rows, reads = random_case()
    best = random_truth()
    read_primer = np.arange(len(reads), dtype=np.int32) // 2
    codes, off = pack_reads(reads)
    lo, hi = 20, 2500
    ctx = hip_lib.context(0)
    try:
        ctx.seq_load(*pack_rows(rows))
        got = {}
        for max_gap in (0, 2, MAX_GAP):
            got[max_gap] = ctx.offtarget_gap_resident(codes, off, read_primer, RANDOM_PEN, max_gap, RANDOM_TERM, lo, hi)
        first, _ = ctx.offtarget_stats()
        again = ctx.offtarget_gap_resident(codes, off, read_primer, RANDOM_PEN, MAX_GAP, RANDOM_TERM, lo, hi, cap=3)
        second, counts = ctx.offtarget_stats()
        ungapped = ctx.offtarget_resident(codes, off, read_primer, RANDOM_PEN // 6, RANDOM_TERM, lo, hi)
        with pytest.raises(MprimeError) as bad:
            ctx.offtarget_gap_resident(codes, off, read_primer, RANDOM_PEN, MAX_GAP + 1, RANDOM_TERM, lo, hi)
    finally:
        ctx.close()
    for max_gap, prod in got.items():
        assert [tuple(x) for x in prod.tolist()] == _expected_products(best, read_primer.tolist(), max_gap, lo, hi), max_gap
    assert len(got[0]) < len(got[2]) <= len(got[MAX_GAP]) and len(got[0]) > 0
    # going past a small cap and calling again returns the kept products: no second scan
    assert len(again) > 3 and again.tolist() == got[MAX_GAP].tolist()
    assert first["scan_ms"] > 0 and second["scan_ms"] == 0 and counts["products"] == len(again)
    assert ungapped.tolist() == got[0].tolist()
    assert bad.value.code == -1                                                      # MP_ERR_ARG


@pytest.mark.gpu
def test_bad_max_gap_is_an_argument_error(hip_lib):
    codes, off = pack_reads([make_read(18)])
    ctx = hip_lib.context(0)
    try:
        ctx.seq_load(*pack_rows(["ACGT" * 50]))
        for max_gap in (-1, MAX_GAP + 1):
            with pytest.raises(MprimeError) as e:
                ctx.kmm_gap_scan_resident(codes, off, 11, max_gap, 1)
            assert e.value.code == -1, max_gap                                       # MP_ERR_ARG
            with pytest.raises(MprimeError) as e:
                ctx.offtarget_gap_resident(codes, off, np.zeros(1, np.int32), 11, max_gap, 1, 100, 1500)
            assert e.value.code == -1, max_gap
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("script", ("primer_coverage_validation_by_BWT.py", "primer_specificity.py"))
def test_drop_in_commands_with_gaps(script, hip_lib, tmp_path):
    """A product whose forward site exists only with a 1-base deletion: a row of the report with --gaps, absent without the flag
    (where the report is what it was: the exact pair on the second sequence alone)."""
    F, R = make_read(18, seed=3), make_read(18, seed=4)
    rng = np.random.default_rng(77)
    gapped = _bases(rng, 300) + site_text(F, "D", 1, 9) + _bases(rng, 150) + rc(R) + _bases(rng, 200)
    exact = _bases(rng, 50) + F + _bases(rng, 182) + rc(R) + _bases(rng, 60)
    (tmp_path / "p.fa").write_text(f">F\n{F}\n>R\n{R}\n")
    (tmp_path / "db.fa").write_text(f">s1\n{gapped}\n>s2\n{exact}\n")
    rows = {}
    for flag in ([], ["--gaps"]):
        out = tmp_path / ("out" + "".join(flag))
        cmd = [sys.executable, os.path.join(REPO, "scripts", script), "-i", str(tmp_path / "p.fa"), "-r", str(tmp_path / "db.fa"),
               "-l", "18", "-t", "4", "-s", "100,1500", "-o", str(out)] + flag
        subprocess.run(cmd, check=True, capture_output=True, timeout=300)
        rows[bool(flag)] = out.read_text().splitlines()[1:]
    assert rows[False] == ["s2\t50\t250\tF\tR\t201"]
    assert sorted(rows[True]) == ["s1\t300\t469\tF\tR\t170", "s2\t50\t250\tF\tR\t201"]


@pytest.mark.gpu
def test_bowtie2_fixture_is_unchanged_with_gaps_on_the_device(hip_lib, tmp_path, capsys):
    """tests/test_gapscan.py::test_bowtie2_fixture_is_unchanged_with_gaps through the device kernel: consistency with the recorded
    bowtie2 run, not evidence for gaps."""
    check_bowtie2_fixture_with_gaps(hip_lib, tmp_path)
    capsys.readouterr()
