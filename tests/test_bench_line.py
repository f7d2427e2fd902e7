"""bench.py's final stdout line is what the driver parses: it must stay one short JSON object (a 20 KB line was not parsed)."""
import importlib.util
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_headline_of_a_recorded_result_is_short_json():
    bench = _bench()
    with open(os.path.join(REPO, "profiles", "r05_bench_default_flags.json")) as f:
        res = json.load(f)                                  # a full result of round 5: 20 KB, every side block present
    assert len(json.dumps(res)) > 16000
    line = bench.headline(res)
    assert len(line) < bench.HEADLINE_LIMIT <= 4096 and "\n" not in line
    out = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline", "cpu_baseline", "parity_checked", "projected_strong_scaling"):
        assert key in out, key
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(out["roofline"])
    assert out["roofline"]["bound"] in ("hbm", "mfma")
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(out["cpu_baseline"])
    assert "workload" in out["config"] and "model" not in out["config"]
    assert abs(out["value"] - res["value"]) <= 1e-5 * res["value"]
    assert abs(out["roofline"]["frac"] - res["roofline"]["frac"]) <= 1e-5


def test_headline_survives_padded_side_blocks():
    bench = _bench()
    with open(os.path.join(REPO, "profiles", "r05_bench_default_flags.json")) as f:
        res = json.load(f)
    res["config"]["workload"] = "w" * 5000
    res["cpu_baseline"]["sample"] = "s" * 5000
    res["roofline"]["kernel"] = "eval_slide_kernel (" + "x" * 5000
    res["pipeline"]["rows_7"] = {"run_ms": 1.0, "construct_ms": 2.0, "tsv_equal_oracle": True, "junk": "j" * 5000}
    line = bench.headline(res)
    assert len(line) < 4096
    json.loads(line)


def test_provisional_headline_is_a_complete_contract_line():
    """bench.py prints the headline once its own fields exist, before the side measurements: a process that dies in one of them leaves
    that line as the last line of stdout.  It carries every key of the contract + roofline + cpu_baseline."""
    bench = _bench()
    with open(os.path.join(REPO, "profiles", "r05_bench_default_flags.json")) as f:
        res = json.load(f)
    for side in ("variants", "pipeline", "weak_shard", "shard_shapes", "k_sweep", "side_steps", "projected_strong_scaling"):
        res.pop(side, None)                                 # what exists when the provisional line is printed
    out = json.loads(bench.headline({**res, "provisional": True}))
    assert out["provisional"] is True
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline", "cpu_baseline", "parity_checked"):
        assert key in out, key
    src = open(os.path.join(REPO, "bench.py")).read()
    assert src.index('"provisional": True') < src.index('progress("variants")') < src.index("emit(res)")


def test_headline_of_a_plain_run_names_no_side_measurement():
    """Without --full bench.py measures the headline alone: its line carries the contract's keys and nothing that a side measurement fills."""
    bench = _bench()
    with open(os.path.join(REPO, "profiles", "r05_bench_default_flags.json")) as f:
        res = json.load(f)
    contract = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
    plain = {key: res[key] for key in contract + ("n_gpus", "steps", "warmup", "scaling", "vs_baseline", "data", "config")}
    plain["steps_in_flight"] = 2
    out = json.loads(bench.headline(plain, detail=False))
    for key in contract:
        assert out[key] == (bench._sig(plain[key]) if isinstance(plain[key], float) else plain[key]), key
    assert not {"roofline", "cpu_baseline", "parity_checked", "projected_strong_scaling", "pipeline", "ms_per_step_one_stream", "detail"} & set(out)
    assert json.loads(bench.headline(res))["detail"] == "bench_detail.json"


def test_side_measurements_wait_for_full():
    bench = _bench()
    assert bench.parse_args(["--steps", "3"]).full is False
    assert bench.parse_args(["--full", "--no-shard"]).full is True


def _fake_child(tmp_path, body):
    path = tmp_path / "child.py"
    path.write_text("import json, os, signal, sys\n" + body)
    return [__import__("sys").executable, str(path)]


def test_supervisor_keeps_the_headline_of_a_child_that_dies_in_a_side_block(tmp_path):
    """bench.py at N = 1 measures in a child process: a fatal signal after the provisional headline leaves that headline as the last line."""
    import io
    bench = _bench()
    line = {"metric": "m", "value": 1.5, "unit": "u", "roofline": {"frac": 0.3}, "cpu_baseline": {"value": 1}, "provisional": True}
    out = io.StringIO()
    rc = bench.supervise(_fake_child(tmp_path, f"print(json.dumps({line!r})); sys.stdout.flush(); print('bench_detail: {{half', end=''); sys.stdout.flush()\n"
                                               "os.kill(os.getpid(), signal.SIGSEGV)\n"), out=out)
    last = json.loads(out.getvalue().splitlines()[-1])
    assert rc == 0 and "provisional" not in last and last["value"] == 1.5 and "side_measurements" in last


def test_supervisor_passes_a_finished_child_through_and_retries_an_early_death(tmp_path):
    import io
    bench = _bench()
    out = io.StringIO()
    final = {"metric": "m", "value": 2.0, "parity_checked": False}
    rc = bench.supervise(_fake_child(tmp_path, f"print(json.dumps({{'metric': 'm', 'value': 1.0, 'provisional': True}}))\nprint('bench_detail: x')\n"
                                               f"print(json.dumps({final!r}))\nsys.exit(1)\n"), out=out)
    assert rc == 1 and json.loads(out.getvalue().splitlines()[-1]) == final          # parity failure: the child's own status
    marker = tmp_path / "second"
    out = io.StringIO()
    rc = bench.supervise(_fake_child(tmp_path, f"p = {str(marker)!r}\nif not os.path.exists(p):\n    open(p, 'w').close(); os.kill(os.getpid(), signal.SIGSEGV)\n"
                                               "print(json.dumps({'metric': 'm', 'value': 3.0}))\n"), out=out)
    assert rc == 0 and json.loads(out.getvalue().splitlines()[-1])["value"] == 3.0


def test_dump_outputs_writes_float64_counters_within_the_limit(tmp_path, monkeypatch):
    import numpy as np
    bench = _bench()
    counters = np.random.default_rng(3).integers(0, 1 << 40, size=(1000, 3), dtype=np.int64)
    bench.dump_outputs(str(tmp_path / "all"), counters)
    got = np.load(tmp_path / "all" / "coverage_counters.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.int64), counters)
    assert not (tmp_path / "all" / "coverage_counters_index.npy").exists()
    monkeypatch.setattr(bench, "DUMP_LIMIT", 100 * 2 * 24)                  # room for 100 candidates and their indices
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), counters)
    idx, got = np.load(tmp_path / "s1" / "coverage_counters_index.npy"), np.load(tmp_path / "s1" / "coverage_counters.npy")
    assert len(idx) == 100 and np.all(np.diff(idx) > 0) and np.array_equal(got.astype(np.int64), counters[idx.astype(np.int64)])
    assert idx.nbytes + got.nbytes <= bench.DUMP_LIMIT
    assert np.array_equal(idx, np.load(tmp_path / "s2" / "coverage_counters_index.npy"))     # the same sample every run


@pytest.mark.gpu
def test_plain_run_prints_one_headline_and_writes_only_the_dump(tmp_path):
    """A plain run on the GPU: exit 0, one stdout line (the headline, no roofline / oracle leg), the counters under --dump-outputs, no detail file."""
    import subprocess
    import sys
    import numpy as np
    detail = os.path.join(REPO, "bench_detail.json")
    before = os.path.getmtime(detail) if os.path.exists(detail) else None
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--rows", "131072",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == "candidate x sequence coverage evals/s" and out["unit"] == "evals/s" and out["dtype"] == "u32"
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["steps"] == 4 and out["warmup"] == 1
    assert not {"roofline", "cpu_baseline", "parity_checked", "detail"} & set(out)
    got = np.load(tmp_path / "out" / "coverage_counters.npy")
    assert got.dtype == np.float64 and got.shape == (out["config"]["windows"] * out["config"]["candidates_per_window"], 3)
    assert (os.path.getmtime(detail) if os.path.exists(detail) else None) == before
