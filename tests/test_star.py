"""The yardstick of the star alignment (tests/star_ref.py, the rule of include/mprime_star.h) checked on its own: what every case of
tests/star_cases.py is meant to provoke does happen, every row is lossless, and a planted family comes back with its planted homology.
Then the same for the cases of tests/star_edge_cases.py, which take the device's kernels past one tile: the bands the records end at and
where the flagged ones stand, the widths, the slots that carry insertions, the unplaced records at the tile boundaries, and the
length-limit case against its planted expectation.  No device is involved."""
import pytest

import star_cases as cases
import star_edge_cases as edges
import star_ref as ref
from anchor_ref import anchor_of


@pytest.fixture(scope="module")
def truth():
    groups = cases.all_groups()
    return {g["name"]: (g, cases.yardstick(g)) for g in groups}


def last(truth, name):
    g, res = truth[name]
    return g, cases.cleaned(g), res, res["rounds"][-1]


def first(truth, name):
    """Round 0: its anchor is the first record of every hand-built group."""
    g, res = truth[name]
    assert res["anchors"][0] == cases.cleaned(g)[0]
    return g, cases.cleaned(g), res, res["rounds"][0]


def test_every_row_is_lossless_and_equally_wide(truth):
    for name, (g, res) in truth.items():
        records = cases.cleaned(g)
        for rnd, anchor in zip(res["rounds"], res["anchors"]):
            assert rnd["width"] == len(anchor) + sum(rnd["ins"]) and len(rnd["ins"]) == len(anchor) + 1, name
            assert any(rnd["placed"]), name
            for q, row, ok, mt in zip(records, rnd["rows"], rnd["placed"], rnd["meta"]):
                assert (row is not None) == ok == (not mt["status"] & 1), name
                if ok:
                    assert len(row) == rnd["width"] and row.replace("-", "") == q, (name, q)
            # the counts are those of the placed rows
            kept = [r for r in rnd["rows"] if r is not None]
            assert all(sum(c) == len(kept) for c in rnd["counts"]), name


def columns_of(row):
    """Column of every base of a row."""
    return [c for c, ch in enumerate(row) if ch != "-"]


@pytest.mark.parametrize("name", ("family1", "family2"))
def test_a_planted_family_recovers_its_homology(truth, name):
    g, records, res, rnd = last(truth, name)
    assert res["anchors"][0] == records[0] and all(rnd["placed"])
    centre = columns_of(rnd["rows"][0])
    gaps_of_centre = {c for c, ch in enumerate(rnd["rows"][0]) if ch == "-"}
    assert sum(1 for h in g["homology"][1:] for x in h if x is None) > 10 and sum(len(h) < len(records[0]) for h in g["homology"]) > 3
    for row, hom in zip(rnd["rows"], g["homology"]):
        for col, p in zip(columns_of(row), hom):
            assert (col in gaps_of_centre) if p is None else (col == centre[p]), (name, row)


def test_two_substitutions_in_the_last_two_bases_realign():
    """Why the planted families keep their ends quiet: with the last base changed into the anchor's second-last one, dropping the base
    before it (an insertion, 12) lets it match one column earlier (+5 for -4) and saves the other mismatch: -7 against -8."""
    import random
    anc = cases.rand_seq(random.Random(4), 60) + "GA"
    rnd = ref.star([anc, anc[5:-2] + "TG"], rounds=1)["rounds"][0]
    assert rnd["meta"][1]["n_ins"] == 1 and rnd["meta"][1]["status"] == 0 and rnd["rows"][1].endswith("TG-")


def test_slot_0_and_slot_n(truth):
    g, records, res, rnd = first(truth, "slot0-slotn")
    n = len(records[0])
    assert rnd["ins"][0] == 3 and rnd["ins"][n] == 3 and sum(rnd["ins"]) == 6
    assert rnd["rows"][1].startswith("TTT") and rnd["rows"][2].startswith("--G") and rnd["rows"][0].startswith("---")
    assert rnd["rows"][3].endswith("GGA") and rnd["rows"][4].endswith(records[4][-1] + "--") and rnd["rows"][0].endswith("---")
    assert (n + 1) % 16 and rnd["width"] % 16


def test_two_records_share_a_slot(truth):
    g, records, res, rnd = first(truth, "same-slot")
    x2, x5 = g["runs"]
    assert rnd["ins"][40] == 5 and sum(rnd["ins"]) == 5
    a = rnd["acol"][40]
    assert rnd["rows"][1][a - 5:a] == x2 + "---" and rnd["rows"][2][a - 5:a] == x5 and rnd["rows"][0][a - 5:a] == "-----"


def test_runs_stay_whole_without_a_gap_open_penalty(truth):
    g, records, res, rnd = first(truth, "gap-open-0")
    x2, x5 = g["runs"]
    n = len(records[0])
    assert g["params"]["gap_open"] == 0 and all(rnd["placed"])
    assert [m["n_ins"] for m in rnd["meta"]] == [0, 2, 5, 3, 3]
    assert rnd["ins"][0] == 3 and rnd["ins"][40] == 5 and rnd["ins"][n] == 3 and sum(rnd["ins"]) == 11
    a = rnd["acol"][40]
    assert rnd["rows"][1][a - 5:a] == x2 + "---" and rnd["rows"][2][a - 5:a] == x5
    assert rnd["rows"][3].startswith("TTT") and rnd["rows"][4].endswith("GGA")


def test_leading_run_right_and_interior_run_left(truth):
    g, records, res, rnd = first(truth, "lead-and-interior")
    lead, x3, x5 = g["runs"]
    assert rnd["ins"][0] == 4 and rnd["ins"][30] == 5 and sum(rnd["ins"]) == 9
    a = rnd["acol"][30]
    assert rnd["rows"][1][:4] == "--" + 2 * lead and rnd["rows"][1][a - 5:a] == x3 + "--"
    assert rnd["rows"][2][:4] == "AC" + 2 * lead and rnd["rows"][2][a - 5:a] == x5


def test_insertion_directly_followed_by_deletion(truth):
    g, records, res, rnd = first(truth, "ins-then-del")
    r = ref.align_escalating(records[1], records[0], 32, **{k: v for k, v in g["params"].items() if k != "band"})[0]
    assert "ID" in r["ops"] and "DI" not in r["ops"]
    assert rnd["ins"][45] == 1 and rnd["rows"][1][rnd["acol"][45] - 1] == records[1][45] and rnd["rows"][1][rnd["acol"][45]] == "-"


def test_an_unplaced_record_widens_nothing(truth):
    g, records, res, rnd = last(truth, "unplaced")
    assert rnd["placed"] == [True, True, False, True] and rnd["meta"][2]["n_ins"] > 0
    without = ref.star([r for q, r in enumerate(records) if q != 2], rounds=g["rounds"], **g["params"])["rounds"][-1]
    assert without["ins"] == rnd["ins"] and without["rows"] == [r for r in rnd["rows"] if r is not None]
    assert sum(rnd["ins"]) == 3


def test_one_record_and_identical_records(truth):
    g, records, res, rnd = last(truth, "single")
    assert rnd["rows"] == records and len(res["anchors"]) == 1 and rnd["width"] == 57
    g, records, res, rnd = last(truth, "identical")
    assert rnd["rows"] == records and len(res["anchors"]) == 1 and len(res["rounds"]) == 1 and rnd["width"] == len(records[0])


def test_gaps_in_the_input_are_removed_first(truth):
    g, records, res, rnd = first(truth, "gapped-input")
    assert all("-" not in r and "." not in r and r == r.upper() for r in records) and len(records[2]) == 47
    assert any("-" in r or "." in r for r in g["records"])
    assert rnd["ins"][20] == 2 and sum(rnd["ins"]) == 2


def test_the_band_grows_for_a_drifting_record(truth):
    for kind in ("ins", "del"):
        g, records, res, rnd = first(truth, f"drift-64-{kind}")
        assert [m["band"] for m in rnd["meta"]] == [32, 64, 32] and all(m["status"] == 0 for m in rnd["meta"]), kind
        n = len(records[0])
        assert ref.align(records[1], records[0], list(range(n)), n, **g["params"])["status"] & 2
        assert (rnd["ins"][100] == 40 and sum(rnd["ins"]) == 40) if kind == "ins" else rnd["meta"][1]["n_del"] == 40
    g, records, res, rnd = first(truth, "drift-255")
    assert [m["band"] for m in rnd["meta"]] == [32, 255, 32] and rnd["meta"][1]["status"] & 2


def test_the_consensus_round(truth):
    g, records, res, rnd = last(truth, "consensus-moves")
    assert res["anchors"][0] == records[0] and "GATTA" in records[0] and len(records[0]) == 115
    assert res["anchors"][1:] == [g["ancestor"]] and g["rounds"] == 3       # the consensus of round 1 is its own anchor: no third round
    assert res["anchors"][1] == anchor_of([r for r in res["rounds"][0]["rows"] if r is not None])[0]
    assert rnd["ins"][50] == 5 and rnd["rows"][0][50:55] == "GATTA"
    g, records, res, rnd = last(truth, "consensus-stays")
    assert len(res["anchors"]) == 1 and g["rounds"] == 3 and all(rnd["placed"])


def test_refusals():
    with pytest.raises(ValueError):
        ref.star(["ACGT", ""])
    with pytest.raises(ValueError):
        ref.star(["A" * (ref.MAX_LEN + 1)])
    assert ref.clean("ac-g.T") == "ACGT" and ref.centre_of(["AC", "ACG", "TTT"]) == 1


# ---- the edge cases of tests/star_edge_cases.py: each provokes on the yardstick what tests/test_star_edges.py runs it for -------------------
def ceil8(record):
    return (len(record) + 7) // 8


@pytest.mark.parametrize("n_records", edges.TINY_SIZES)
def test_many_tiny_records_flag_fixed_positions_and_end_at_four_bands(n_records):
    g = edges.many_tiny(n_records)
    rnd, plan, runs = edges.yardstick_round(g), g["plan"], g["runs"]
    records, bands = cases.cleaned(g), [m["band"] for m in rnd["meta"]]
    assert len(records) == n_records and g["params"]["band"] == 4 and plan["per"] == {256: 1, 257: 1, 1024: 1, 1025: 2, 2049: 3}[n_records]
    assert len(records[0]) == 48 and all(20 <= len(r) <= 60 for r in records[1:])
    # every record ends at the band its run was chosen for; the strangers are unplaced and nothing else is
    for q in range(n_records):
        if q in plan["strangers"]:
            assert not rnd["placed"][q] and set(records[q]) <= set("AG"), q
        else:
            assert bands[q] == edges.TINY_BAND_OF_RUN[runs[q]] if q in runs else bands[q] == 4, q
            assert rnd["placed"][q] and rnd["meta"][q]["status"] == 0 and rnd["meta"][q]["n_ins"] == runs.get(q, 0), q
    per_band = {W: sum(1 for q, b in enumerate(bands) if b == W and q not in plan["strangers"]) for W in (4, 8, 16, 32)}
    assert per_band == {W: sum(1 for q in range(n_records) if q not in plan["strangers"] and edges.TINY_BAND_OF_RUN[runs.get(q, 3)] == W)
                        for W in (4, 8, 16, 32)}
    assert all(per_band[W] >= 5 for W in (8, 16, 32)) and per_band[4] > n_records // 2
    assert sum(1 for q in runs if runs[q] == 3) >= 3 and sum(1 for x in rnd["ins"] if x) >= 10
    # the flagged records where the flag scan's slices meet: 1..4, around the first record of three threads, the last records, one whole slice
    per = plan["per"]
    flagged = {q for q, b in enumerate(bands) if b > 4}
    assert plan["flagged"] <= flagged and {1, 2, 3, 4} <= flagged and set(plan["full"]) <= flagged and len(plan["full"]) == per
    assert all({per * t - 1, per * t, per * t + 1} <= flagged for t in plan["threads"])
    assert {n_records - 3, n_records - 2, n_records - 1} - plan["strangers"] <= flagged and len(runs) > n_records // 10
    if n_records >= 1024:
        quiet = plan["quiet"]
        assert len(quiet) == 200 * per and quiet[0] % per == 0 and not flagged & set(quiet)
    # a profile workgroup (256 records) and a count workgroup (1024) start and end on an unplaced record
    assert {q for q in (255, 256, 1023, 1024) if q < n_records} <= plan["strangers"]
    if n_records >= 1024:
        # a count lane reads every fourth row of the first 1024: one of them sees 256 gaps in an inserted column
        lanes = [rl for rl in range(4) if all(rnd["placed"][r] for r in range(rl, 1024, 4))]
        assert any(all(rnd["rows"][r][c] == "-" for r in range(rl, 1024, 4)) for rl in lanes for c in range(rnd["width"]))


def test_rows_narrower_than_sixteen_bytes():
    g = edges.one_letter()
    rnd = edges.yardstick_round(g)
    assert rnd["width"] == 1 and rnd["ins"] == [0, 0] and len(g["records"]) == 1030
    assert [q for q, ok in enumerate(rnd["placed"]) if not ok] == [1024] and rnd["counts"] == [[1029, 0, 0, 0, 0, 0]]
    g = edges.short_rows()
    rnd, records = edges.yardstick_round(g), g["records"]
    assert rnd["width"] == 7 and rnd["ins"] == [2, 0, 0, 0, 0, 0] and sorted({len(r) for r in records}) == [1, 2, 3, 4, 5]
    assert rnd["rows"][records.index("ACG")] == "--ACG--" and rnd["rows"][records.index("GGACG")] == "GGACG--"
    q = records.index("TTTTT")
    assert not rnd["placed"][q] and rnd["placed"].count(False) == 1 and 0 < q < len(records) - 1 and 16 // 7 >= 2       # a lane spans three rows
    g = edges.width15()
    rnd = edges.yardstick_round(g)
    assert rnd["width"] == 15 and rnd["ins"][0] == 2 and sum(rnd["ins"]) == 2 and (len(g["records"]) * 15) % 16
    assert any(not rnd["placed"][q] and rnd["placed"][q - 1] and rnd["placed"][q + 1] for q in range(1, len(g["records"]) - 1))
    assert rnd["placed"][0] and rnd["placed"][-1]


@pytest.fixture(scope="module")
def long_truth():
    return {g["name"]: (g, edges.yardstick_round(g)) for g in edges.long_groups()}


@pytest.mark.parametrize("n", edges.LONG_SIZES)
def test_long_anchors_carry_insertions_where_the_tiles_meet(long_truth, n):
    g, rnd = long_truth[f"long{n}"]
    records, plan, per = cases.cleaned(g), g["plan"], g["per"]
    assert len(records[0]) == n and per == (n + 1 + 1023) // 1024 == {1023: 1, 1024: 2, 2047: 2, 2048: 3, 2100: 3}[n]
    assert {j: x for j, x in enumerate(rnd["ins"]) if x} == plan and all(rnd["placed"]) and all(m["band"] == 32 for m in rnd["meta"])
    assert {0, n} | {j for j in (1023, 1024, 2047, 2048) if j <= n} <= set(plan) and len(plan) >= 12 + 2
    # slices of the column scan with an insertion in their first and in their last slot
    assert len(g["threads"]) >= 6 and all(rnd["ins"][per * t] and rnd["ins"][per * t + per - 1] for t in g["threads"])
    assert rnd["width"] == n + sum(plan.values()) and rnd["rows"][1].startswith(records[1][:plan[0]])
    assert rnd["rows"][-1].endswith(records[-1][-plan[n]:]) and rnd["rows"][0].endswith("-" * plan[n])
    for a, b in zip(records, records[1:]):
        assert a != b and ceil8(a) != ceil8(b)
    assert all(1 <= len(h) <= 2 for h in g["held"]) and all(150 <= len(r) <= 400 for r in records[1:])


def test_widths_1024_and_1025(long_truth):
    for width in (1024, 1025):
        g, rnd = long_truth[f"width{width}"]
        assert len(g["anchor"]) == 1000 and rnd["width"] == width and {j: x for j, x in enumerate(rnd["ins"]) if x} == g["plan"]
        assert rnd["ins"][0] == 3 and rnd["ins"][1000] == 3 and all(rnd["placed"])


def test_every_record_of_the_chunked_list_is_aligned_again():
    g = edges.chunked_list()
    rnd, records = edges.yardstick_round(g), cases.cleaned(g)
    assert len(records) == 45 and ref.centre_of(records) == 0 and records[0] == g["anchor"] and g["params"]["band"] == 32
    assert [m["band"] for m in rnd["meta"]] == [{0: 32, 1: 64, 2: 128}[k] for k in g["kinds"]]
    assert g["kinds"].count(1) == 29 and g["kinds"].count(2) == 15 and all(m["status"] == 0 for m in rnd["meta"])
    assert len(set(records)) == 45 and all(ceil8(a) != ceil8(b) for a, b in zip(records, records[1:]))
    assert all(m["n_del"] == {0: 0, 1: 40, 2: 70}[k] for m, k in zip(rnd["meta"], g["kinds"]))
    # at four diagonals per lane (W = 64) the list takes more words than the whole batch at two (W = 32)
    assert edges.flagged_words(g, rnd, 0, 45, 4) > sum(ceil8(r) * 128 for r in records)


def test_the_length_limit_case_is_what_the_rule_gives():
    case = edges.limit_case(3000)
    anchor, records = case["anchor"], case["records"]
    assert [len(r) for r in records] == [3000, 3000, case["b"] - 100 + 3] and case["a"] - 100 > case["b"] - case["a"] and case["substitutions"] > 40
    rnd = ref.star_round(records, anchor)
    for key in ("rows", "meta", "ins", "width", "counts", "placed"):
        assert rnd[key] == case["star"][key], key
    from anchor_ref import align
    for q, want in zip(records[1:], case["anchored"]):
        got = align(q, anchor, list(range(3000)), 3000)
        assert {k: got[k] for k in want} == want
