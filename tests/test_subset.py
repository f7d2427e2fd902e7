"""The global-optimum degenerate positions (`-m multiPrime2`) without a GPU: the plain-Python model of tests/subset_ref.py against the
recorded calls of the reference's get_Y_position (tests/golden/subset_msa1000.json.gz, made by tests/golden/make_golden_subset.py), the
host replay of the library (mp_subset_replay / mp_subset_choose: no device) fed with the model's per-step results, and the refusals of the
command line."""
import random

import numpy as np
import pytest

import subset_ref as ref
from conftest import load_gz_json


@pytest.fixture(scope="module")
def golden():
    return load_gz_json("subset_msa1000.json.gz")


def calls_of(golden):
    return golden["windows"] + golden["direct"]


def test_fixture_holds_what_it_should(golden):
    wins = golden["windows"]
    assert {(c["N"], c["v"]) for c in wins} == {(4, 1), (3, 2)}
    assert sum(c["role"] == "NM" for c in wins) == sum(c["role"] == "MM" for c in wins) > 10
    assert sum(c["role"] == "one" for c in wins) > 20
    short = 0
    for c in wins:
        recs = ref.records(c["seed"], c["cover"])
        short += any(len(ref.step(recs, dn, c["v"], c["cover_number"])[0]) < dn for dn in range(2, c["N"] + 1))
    assert short >= 3                                        # the |T| < dn rule
    exits = 0
    for c in golden["direct"]:
        assert all(n == 1 for _, n in c["cover"]) and c["cover_number"] == len(c["cover"])
        recs = ref.records(c["seed"], c["cover"])
        exits += any(ref.step(recs, dn, c["v"], c["cover_number"])[4] >= 0 for dn in range(2, c["N"] + 1))
    assert exits >= 4                                        # the early exit, which the sample alignment never takes


def test_model_equals_every_recorded_call(golden):
    for c in calls_of(golden):
        subset, count, primer = ref.select(c["seed"], c["cover"], c["cover_number"], c["N"], c["v"])
        assert (primer, count) == (c["primer"], c["count"]), (c.get("position"), c["role"], c["seed"], subset)


def test_model_does_not_depend_on_the_order_of_cover(golden):
    rng = random.Random(7)
    for c in calls_of(golden)[::3]:
        items = list(c["cover"])
        rng.shuffle(items)
        assert ref.select(c["seed"], items, c["cover_number"], c["N"], c["v"]) == ref.select(c["seed"], c["cover"], c["cover_number"], c["N"], c["v"])


def model_steps(calls):
    """The per-step results of the library's search as the model computes them: arrays [n][N - 1](...) (all calls share N)."""
    N = calls[0]["N"]
    n, st = len(calls), N - 1
    out = {"t_mask": np.zeros((n, st, 2), np.uint64), "n_admitted": np.zeros((n, st), np.int32), "best_total": np.zeros((n, st), np.int64),
           "best_rank": np.full((n, st), -1, np.int64), "exit_rank": np.full((n, st), -1, np.int64), "pre_total": np.zeros((n, st), np.int64)}
    for i, c in enumerate(calls):
        recs = ref.records(c["seed"], c["cover"])
        for dn in range(2, N + 1):
            T, n_adm, best, best_rank, exit_rank, pre = ref.step(recs, dn, c["v"], c["cover_number"])
            out["t_mask"][i, dn - 2] = ref.mask_of(T)
            out["n_admitted"][i, dn - 2] = n_adm
            if len(T) >= dn:
                out["best_total"][i, dn - 2], out["best_rank"][i, dn - 2] = best, best_rank
                out["exit_rank"][i, dn - 2], out["pre_total"][i, dn - 2] = exit_rank, pre
    return out


def seeds_of(calls):
    return np.array([["ACGT".index(ch) for ch in c["seed"]] for c in calls], np.uint8)


def test_host_replay_returns_the_models_subset(golden):
    from multiprime_amd import host, iupac, subset
    groups = {}
    for c in calls_of(golden):
        groups.setdefault((len(c["seed"]), c["N"]), []).append(c)
    for (k, N), calls in groups.items():
        steps = model_steps(calls)
        masks, counts, codes = subset.replay(host.dll(), k, N, seeds_of(calls), [c["cover_number"] for c in calls], steps)
        primers = iupac.strings_of(iupac.SYMBOL_LUT[codes])
        for i, c in enumerate(calls):
            want, count, primer = ref.select(c["seed"], c["cover"], c["cover_number"], N, c["v"])
            assert tuple(int(x) for x in masks[i]) == ref.mask_of(want), (i, c["seed"])
            assert (primers[i], int(counts[i])) == (primer, count) == (c["primer"], c["count"])


def test_host_choice_between_the_seeds(golden):
    from multiprime_amd import host, subset
    wins = golden["windows"]
    pairs = [(i, i + 1) for i, c in enumerate(wins) if c["role"] == "NM"]
    assert all(wins[b]["role"] == "MM" and wins[b]["position"] == wins[a]["position"] for a, b in pairs)
    counts = [c["count"] for c in wins]
    chosen = subset.choose(host.dll(), [a for a, _ in pairs] + [0], [b for _, b in pairs] + [-1], counts)
    for (a, b), got in zip(pairs, chosen):
        nm, mm = (None, wins[a]["count"], wins[a]["primer"]), (None, wins[b]["count"], wins[b]["primer"])
        assert wins[int(got)]["primer"] == ref.pick(nm, mm)[2]
    assert chosen[-1] == 0
    assert subset.choose(host.dll(), [0], [1], [5, 5]).tolist() == [0] and subset.choose(host.dll(), [0], [1], [5, 6]).tolist() == [1]


@pytest.mark.parametrize("extra,message", [(["-l", "33"], "at most 32 bases"), (["--ngpu", "2"], "runs on one GPU"),
                                           (["--grid", "1x2"], "runs on one GPU")])
def test_cli_refuses_what_method_2_does_not_cover(extra, message, capsys):
    from multiprime_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["-i", "in.msa", "-o", "out.tsv", "-m", "multiPrime2"] + extra)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_cli_method_flag_defaults_to_the_chain():
    from multiprime_amd import cli
    assert cli.parse_args(["-i", "a", "-o", "b"]).method == "multiPrime1"
    assert cli.parse_args(["-i", "a", "-o", "b", "-m", "multiPrime2", "-l", "32"]).method == "multiPrime2"
    with pytest.raises(SystemExit):
        cli.parse_args(["-i", "a", "-o", "b", "-m", "multiPrime3"])
