"""The star alignment's assembly kernels and its batching past one tile (csrc/star.hip), on the cases of tests/star_edge_cases.py: one round
on the device against the yardstick of tests/star_ref.py — rows byte for byte, meta with the band, ins, width, counts, placed and the
anchor the counts lead to.  tests/test_star.py checks without a device that every case provokes what it is run for here:
  tiny N       the flag scan with 1, 2 and 3 records per thread and flagged records where its slices meet; more than one workgroup of the
               profile (256 records) and of the count kernel (1024 records), each starting and ending on an unplaced record; a count
               lane's 16-bit counter at 256
  one-letter, width7, width15
               rows narrower than a writer lane's 16 bytes, unplaced ones among them; L' = 1
  long n       the column scan with 1, 2 and 3 slots per thread and insertions in the first and last slot of a slice, in slot 0 and slot n;
               a second column tile of the profile (slot 2048) and of the map and count kernels; L' = 1024 and 1025
  chunked      a flagged list whose traceback words do not fit the buffer: the chunk loop and its offsets, twice in a row
  limit        records of ANCHOR_MAX_LEN bases: one wave per workgroup in the sweep, the vote histogram beyond 64 KiB"""
import pytest

import star_edge_cases as edges
from multiprime_amd._abi import ANCHOR_MAX_LEN
from test_star_gpu import device_round, pack, same_round


def one_round(hip_lib, g):
    """(the round as the yardstick's dict, the device's counters) of a group against its anchor."""
    ctx = hip_lib.context(0)
    try:
        ctx.star_load(*pack(edges.cleaned(g)))
        return device_round(ctx, g["anchor"], g["params"]), ctx.star_stats()[1]
    finally:
        ctx.close()


def realigned(g, rnd):
    """Alignments beyond the first band: one per doubling."""
    return sum(edges.LEVELS[m["band"]] - edges.LEVELS[g["params"]["band"]] for m in rnd["meta"])


@pytest.mark.gpu
@pytest.mark.parametrize("n_records", edges.TINY_SIZES)
def test_many_tiny_records(n_records, hip_lib, monkeypatch):
    monkeypatch.delenv("MP_STAR_BATCH", raising=False)
    g = edges.many_tiny(n_records)
    want = edges.yardstick_round(g)
    got, stats = one_round(hip_lib, g)
    same_round(got, want, g["name"])
    assert stats["batches"] == 1 and stats["realigned"] == realigned(g, want) and stats["placed"] == want["placed"].count(True)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", (edges.one_letter, edges.short_rows, edges.width15))
def test_rows_narrower_than_a_writer_lane(builder, hip_lib):
    g = builder()
    got, stats = one_round(hip_lib, g)
    same_round(got, edges.yardstick_round(g), g["name"])


@pytest.fixture(scope="module")
def long_groups():
    return {g["name"]: g for g in edges.long_groups()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", [f"long{n}" for n in edges.LONG_SIZES] + ["width1024", "width1025"])
def test_long_anchors(name, hip_lib, long_groups):
    g = long_groups[name]
    got, stats = one_round(hip_lib, g)
    same_round(got, edges.yardstick_round(g), name)
    assert stats["realigned"] == 0


@pytest.mark.gpu
def test_a_flagged_list_longer_than_the_traceback_buffer(hip_lib, monkeypatch):
    """One batch of 45 records of which 44 are aligned again at W = 64 and 15 of those once more at 128.  That the list did not fit one
    chunk is taken from the device's own report: the words of the listed records at the wider band exceed the traceback buffer.  At
    W = 64 a lane holds four diagonals (bandsweep.hpp: 2 W + 1 = 129 > 128), so eight rows take 64 x 4 words — twice the 64 x 2 of W = 32,
    by which the buffer of one batch is sized.  (Counted at two diagonals per lane the listed records could never exceed a buffer that
    holds the whole batch at two.)  Then the same with batches of 16, whose lists are chunked as well."""
    g = edges.chunked_list()
    want = edges.yardstick_round(g)
    monkeypatch.delenv("MP_STAR_BATCH", raising=False)
    got, stats = one_round(hip_lib, g)
    assert stats["batches"] == 1 and 4 * edges.flagged_words(g, want, 0, 45, 4) > stats["traceback_bytes"]
    same_round(got, want, g["name"])
    assert stats["realigned"] == realigned(g, want) == 44 + 15
    monkeypatch.setenv("MP_STAR_BATCH", "16")
    got16, stats16 = one_round(hip_lib, g)
    assert stats16["batches"] == 3 and stats16["realigned"] == stats["realigned"]
    assert all(4 * edges.flagged_words(g, want, q0, q0 + 16, 4) > stats16["traceback_bytes"] for q0 in (0, 16, 32))
    assert got16 == got


@pytest.mark.gpu
def test_three_records_at_the_length_limit(hip_lib, monkeypatch):
    """The expectation comes from the planted homology (edges.limit_case; tests/test_star.py holds the yardstick to it at 3000 bases)."""
    monkeypatch.delenv("MP_STAR_BATCH", raising=False)
    case = edges.limit_case(ANCHOR_MAX_LEN)
    assert len(case["anchor"]) == ANCHOR_MAX_LEN == 32767
    ctx = hip_lib.context(0)
    try:
        ctx.star_load(*pack(case["records"]))
        got = device_round(ctx, case["anchor"], {})
        stats = ctx.star_stats()[1]
    finally:
        ctx.close()
    same_round(got, case["star"], "limit")
    assert stats["batches"] == 1 and stats["realigned"] == 0 and stats["placed"] == 3
