"""Runs a list of device jobs of tests/test_ont_gpu.py in one child process, so that the GPU work of the module sits under one time limit
of its own and a fault ends the child, not the test session.
    python tests/ont_device_jobs.py jobs.json results.json
A job: {"name", "env": {NAME: value or null}, "keys": [str] or null (null: keep what is resident), "pieces": [str]}.  Its result:
{"key": [int], "m": [int], "stats": [ms, counts]} or {"error": message}.  The environment is set before each job: the library reads
its switches per call."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multiprime_amd import ontprimer as op  # noqa: E402
from multiprime_amd._abi import Library, MprimeError  # noqa: E402


def main(jobs_path, out_path):
    jobs = json.load(open(jobs_path))
    q = op.rank_table()
    ctx = Library().context(0)
    results = {}
    try:
        for job in jobs:
            for name, value in job.get("env", {}).items():
                if value is None:
                    os.environ.pop(name, None)
                else:
                    os.environ[name] = value
            try:
                if job.get("fresh"):
                    ctx.close()
                    ctx = Library().context(0)
                if job["keys"] is not None:
                    ctx.ont_set_keys(*op.pack(job["keys"]))
                key, m = ctx.ont_assign(*op.pack(job["pieces"]), q)
                results[job["name"]] = {"key": key.tolist(), "m": m.tolist(), "stats": list(ctx.ont_stats())}
            except MprimeError as e:
                results[job["name"]] = {"error": str(e)}
    finally:
        ctx.close()
    json.dump(results, open(out_path, "w"))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
