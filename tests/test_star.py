"""The yardstick of the star alignment (tests/star_ref.py, the rule of include/mprime_star.h) checked on its own: what every case of
tests/star_cases.py is meant to provoke does happen, every row is lossless, and a planted family comes back with its planted homology.
No device is involved."""
import pytest

import star_cases as cases
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
