"""The read-to-primer assignment on the device (csrc/ont.hip behind mp_ont_set_keys / mp_ont_assign) against difflib itself
(tests/ont_ref.py) on the cases of tests/ont_cases.py: the (key index, M) of every piece, integers, no piece left out; then both
scripts end to end on the reference's recorded run.  Every device job of the module runs in one child process under a time limit
(tests/ont_device_jobs.py), the scripts in children of their own."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ont_cases as cases
import ont_ref as ref
from conftest import REPO, load_gz_json

SCRIPTS = {"FindONTprimerV3.py": os.path.join(REPO, "scripts", "FindONTprimer.py"),
           "FindONTexpandprimer.py": os.path.join(REPO, "scripts", "FindONTexpandprimer.py")}
BASE = {"MP_ONT_KEYS_PER_BLOCK": None, "MP_ONT_PRUNE": None, "MP_ONT_WORD": None}
SWITCHES = {"plain": BASE,
            "split": dict(BASE, MP_ONT_KEYS_PER_BLOCK="7"),                          # 150 keys: 22 splits, combined by atomicMax
            "noprune": dict(BASE, MP_ONT_PRUNE="0"),
            "split_noprune": dict(BASE, MP_ONT_KEYS_PER_BLOCK="64", MP_ONT_PRUNE="0"),
            "word64": dict(BASE, MP_ONT_WORD="64")}                                  # 64-bit masks where 32-bit ones would do


@pytest.fixture(scope="module")
def truth():
    """difflib's rounded ratio and match count of every (piece, key) of the pool, computed once."""
    pieces, keys = cases.pool()
    ratio, count = ref.matrix(pieces, keys)
    return pieces, keys, np.array(ratio), np.array(count)


def winners(truth, n_pieces, n_keys):
    """(key index, M) per piece among the first n_keys keys: the first index that reaches the highest rounded ratio."""
    _, _, ratio, count = truth
    idx = np.argmax(ratio[:n_pieces, :n_keys], axis=1)
    return idx.tolist(), count[np.arange(n_pieces), idx].tolist()


def short_part(truth):
    """The pool's pieces and keys of at most 32 bytes — a launch on 32-bit masks — and their winners among themselves."""
    pieces, keys, ratio, count = truth
    pi = [i for i, p in enumerate(pieces) if len(p) <= 32]
    ki = [i for i, k in enumerate(keys) if len(k) <= 32]
    idx = np.argmax(ratio[np.ix_(pi, ki)], axis=1)
    return [pieces[i] for i in pi], [keys[i] for i in ki], idx.tolist(), count[pi, np.array(ki)[idx]].tolist()


@pytest.fixture(scope="module")
def device(hip_lib, truth, tmp_path_factory):
    """Every device job of the module, run once in a child process."""
    assert hip_lib.backend == "hip" and hip_lib.ont
    pieces, keys = truth[0], truth[1]
    jobs = [{"name": "before_keys", "env": SWITCHES["plain"], "keys": None, "pieces": ["ACGT"]}]
    for nk in cases.KEY_COUNTS:
        for i, n in enumerate(cases.PIECE_COUNTS):
            jobs.append({"name": "counts_%d_%d" % (n, nk), "env": SWITCHES["plain"], "keys": keys[:nk] if i == 0 else None, "pieces": pieces[:n]})
    for name, env in SWITCHES.items():
        jobs.append({"name": "pool_" + name, "env": env, "keys": keys, "pieces": pieces, "fresh": name == "plain"})
    short_pieces, short_keys = short_part(truth)[:2]
    for name, env in SWITCHES.items():
        jobs.append({"name": "short_" + name, "env": env, "keys": short_keys, "pieces": short_pieces})
    edge_pieces, edge_keys = cases.word_edge()
    jobs.append({"name": "edge32", "env": BASE, "keys": edge_keys, "pieces": edge_pieces})
    jobs.append({"name": "edge32_split", "env": SWITCHES["split"], "keys": None, "pieces": edge_pieces})
    jobs.append({"name": "edge33", "env": BASE, "keys": None, "pieces": edge_pieces + ["C" * 33]})          # one longer piece: 64-bit masks
    for i, (tp, tk, _, _) in enumerate(cases.tie_cases()):
        for name in ("plain", "split"):
            jobs.append({"name": "tie_%d_%s" % (i, name), "env": dict(SWITCHES[name], MP_ONT_KEYS_PER_BLOCK="1" if name == "split" else None), "keys": tk, "pieces": tp})
    jobs.append({"name": "bad_key", "env": SWITCHES["plain"], "keys": ["ACGT", "ACGN"], "pieces": ["ACGT"]})
    jobs.append({"name": "kept_keys", "env": SWITCHES["plain"], "keys": None, "pieces": ["AAAAAAAAAA"]})
    jobs.append({"name": "long_key", "env": SWITCHES["plain"], "keys": ["A" * 65], "pieces": ["ACGT"]})
    jobs.append({"name": "long_piece", "env": SWITCHES["plain"], "keys": None, "pieces": ["ACGT", "C" * 65]})
    jobs.append({"name": "no_pieces", "env": SWITCHES["plain"], "keys": None, "pieces": []})
    td = tmp_path_factory.mktemp("ont_device")
    json.dump(jobs, open(td / "jobs.json", "w"))
    res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "ont_device_jobs.py"), str(td / "jobs.json"), str(td / "results.json")],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.load(open(td / "results.json"))


@pytest.mark.gpu
@pytest.mark.parametrize("n_keys", cases.KEY_COUNTS)
def test_lane_and_wave_edges(n_keys, device, truth):
    for n in cases.PIECE_COUNTS:
        got = device["counts_%d_%d" % (n, n_keys)]
        assert (got["key"], got["m"]) == winners(truth, n, n_keys), (n, n_keys)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_pool_equals_difflib(switch, device, truth):
    """300 pieces x 150 keys, lengths 0 .. 64 mixed in one launch, N, lower case and the newline among the piece bytes: the plain
    launch, the key list split over workgroups, and both without the pruning bound."""
    got = device["pool_" + switch]
    want = winners(truth, cases.N_PIECES, cases.N_KEYS)
    for p in range(cases.N_PIECES):
        assert (got["key"][p], got["m"][p]) == (want[0][p], want[1][p]), (switch, p, truth[0][p])
    assert got["stats"][1]["keys"] == cases.N_KEYS and got["stats"][1]["pieces"] == cases.N_PIECES and got["stats"][0]["assign_ms"] > 0
    assert sorted({len(p) for p in truth[0]} & {0, 1, 18, 63, 64}) == [0, 1, 18, 63, 64] and {len(k) for k in truth[1]} == {1, 17, 18, 20, 64}


@pytest.mark.gpu
@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_short_strings_on_32_bit_masks(switch, device, truth):
    """No piece and no key above 32 bytes: the kernel form on 32-bit masks (its stack has 17 entries), and with MP_ONT_WORD=64 the
    64-bit form on the same input."""
    pieces, keys, want_key, want_m = short_part(truth)
    assert len(pieces) > 200 and len(keys) > 140 and max(map(len, pieces)) > 20 and "" in pieces
    got = device["short_" + switch]
    for p in range(len(pieces)):
        assert (got["key"][p], got["m"][p]) == (want_key[p], want_m[p]), (switch, p, pieces[p])


@pytest.mark.gpu
def test_edge_of_the_32_bit_form(device):
    """Pieces and keys of 30 .. 32 bytes (shifts by up to 31, runs that end at bit 31); one piece of 33 bytes moves the launch to the
    64-bit form and nothing else changes."""
    pieces, keys = cases.word_edge()
    assert max(map(len, pieces)) == 32 == max(map(len, keys)) and min(map(len, pieces)) >= 1
    ratio, count = ref.matrix(pieces + ["C" * 33], keys)
    idx = np.argmax(np.array(ratio), axis=1)
    want = (idx.tolist(), np.array(count)[np.arange(len(idx)), idx].tolist())
    for name in ("edge32", "edge32_split"):
        assert (device[name]["key"], device[name]["m"]) == (want[0][:-1], want[1][:-1]), name
    assert (device["edge33"]["key"], device["edge33"]["m"]) == want


@pytest.mark.gpu
def test_ties_go_to_the_first_index(device):
    for i, (pieces, keys, want, what) in enumerate(cases.tie_cases()):
        by_difflib = [ref.winner_difflib(p, keys) for p in pieces]
        assert [w[0] for w in by_difflib] == want, what
        for name in ("plain", "split"):
            got = device["tie_%d_%s" % (i, name)]
            assert list(zip(got["key"], got["m"])) == by_difflib, (what, name)
    a, keys = "A" * 10, cases.tie_cases()[0][1]
    assert ref.ratio(a, keys[1]) == ref.ratio(a, keys[2]) and ref.difflib_count(a, keys[1]) != ref.difflib_count(a, keys[2])


@pytest.mark.gpu
def test_refusals(device):
    assert "mp_ont_set_keys first" in device["before_keys"]["error"]
    assert "key 1" in device["bad_key"]["error"] and "0x4E" in device["bad_key"]["error"]
    tie = cases.tie_cases()[-1]                                          # the list set before the refused one is still resident
    assert device["kept_keys"]["key"] == [ref.winner_difflib("AAAAAAAAAA", tie[1])[0]]
    assert "key 0 has 65 bytes" in device["long_key"]["error"]
    assert "piece 1 has 65 bytes" in device["long_piece"]["error"]
    assert device["no_pieces"]["key"] == []


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["v3_fq", "v3_fq_gz", "v3_fa", "v3_fa_gz", "expand_fq"])
def test_scripts_end_to_end(case, hip_lib, tmp_path):
    """Every recorded case of the reference through the drop-in script, in three batches: the recorded lines (ties ordered) and the
    expand file's bytes."""
    golden = load_gz_json("ont_small.json.gz")
    rec = golden["cases"][case]
    with open(tmp_path / golden["primer_file"], "w") as f:
        f.write(golden["primers"])
    for name, text in golden["inputs"].items():
        with open(tmp_path / name, "w") as f:
            f.write(text)
        with gzip.open(tmp_path / (name + ".gz"), "wb") as f:
            f.write(text.encode())
    res = subprocess.run([sys.executable, SCRIPTS[rec["script"]]] + rec["flags"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, MP_ONT_BATCH="15"))
    assert res.returncode == 0, res.stderr[-3000:]
    assert "Total times" in res.stdout and "%d pieces" % (2 * len(cases.golden_reads())) in res.stdout
    assert open(tmp_path / (case + ".num")).readlines() == ref.order_lines(rec["lines"])
    assert open(tmp_path / rec["expand_file"]).read() == rec["expand_text"]
