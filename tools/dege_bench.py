#!/usr/bin/env python3
"""DegePrime on the device (profiles/dege.txt): what mp_dege_stats says for the window stage and the merging, and the wall time of the
whole tool, on the recorded 150 x 320 slice (tests/golden/dege.json.gz, -l 18 -d 12) and on a synthetic alignment.

    python tools/dege_bench.py [--rows 100000 --cols 1000 --seed 7 -l 18 -d 12 --iter 100]     (needs the GPU)

The synthetic alignment is multiprime_amd/synth.py's block (substitutions, gaps, ragged edges, a few IUPAC letters) as it is: no
trimming, so every letter is upper case."""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from multiprime_amd.degeprime import DegePrime, main as run_dege  # noqa: E402
from multiprime_amd.synth import synth_block  # noqa: E402


def report(name, job, rows, repeats=3):
    for k in range(repeats):
        t0 = time.time()
        text = job.table(rows)
        wall = time.time() - t0
        ms, counts = job.stats
        total = sum(int(line.split("\t")[6]) for line in text.splitlines()[1:])
        print("%s run %d: %d x %d, window_ms %.3f merge_ms %.3f, windows %d printed %d unique %d global-table windows %d, summed NumberMatching %d, "
              "table() wall %.3f s" % (name, k, rows.shape[0], rows.shape[1], ms["window_ms"], ms["merge_ms"], counts["windows"], counts["printed"],
                                       counts["unique"], counts["global_windows"], total, wall))


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=100000)
    p.add_argument("--cols", type=int, default=1000)
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("-l", type=int, default=18)
    p.add_argument("-d", type=int, default=12)
    p.add_argument("--iter", type=int, default=100)
    a = p.parse_args()
    g = json.loads(gzip.open(os.path.join(REPO, "tests", "golden", "dege.json.gz")).read())["dege_sub"]
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "trim.fa")
        open(path, "w").write(g["trim"])
        t0 = time.time()
        run_dege(["-i", path, "-o", os.path.join(td, "table.txt"), "-l", str(g["flags"]["l"]), "-d", str(g["flags"]["d"])])
        print("dege_sub: run_dege.py's main from a cold library %.3f s (DegePrime.pl on the CPU: %.1f s)" % (time.time() - t0, g["perl_seconds"]))
        from multiprime_amd.degeprime import read_trimmed
        report("dege_sub", DegePrime(length=g["flags"]["l"], deg=g["flags"]["d"]), read_trimmed(path))
    rows = synth_block(0, a.rows, a.cols, a.seed)
    report("synthetic", DegePrime(length=a.l, deg=a.d, iters=a.iter), rows, repeats=2)
