#!/usr/bin/env python3
"""get_Maxprimerset -r measured: the greedy set cover with the off-target test on a synthetic background, one JSON line per measurement.

    python tools/setscreen_bench.py                      # on the GPU box: run() with -r, run() without -r, the model's rate on a slice

Per add of the examiner (device event times, mp_setscreen_stats): the first add (the first --lookahead pairs of every cluster in one batch)
and the median / maximum over the later ones (the next pairs of one cluster).  Input: the background generator of tools/panel_bench.py (synth.offtarget_case: uniform-random rows of --row-len bases, --bases in all)
and --clusters clusters of --pairs pairs of random 20-base primers, every fourth reverse primer with one R eight bases from its end.
The `model` line times tests/setscreen_ref.py (pure Python) on ONE primer and a --model-bases slice; `scaled_s` is that time scaled
linearly by reads x bases to the full input and is labelled as scaled: the model was not run at that size.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def candidates(path, n_clusters, n_pairs, seed):
    rng = np.random.default_rng(seed)
    primers = []
    with open(path, "w") as f:
        for c in range(n_clusters):
            row = [f"cluster{c}"]
            for j in range(n_pairs):
                fw, rv = ("".join("ACGT"[i] for i in rng.integers(0, 4, 20)) for _ in range(2))
                if j % 4 == 3:
                    rv = rv[:12] + "R" + rv[13:]
                primers += [fw, rv]
                row += [fw, rv, "300:60.0:1", str(n_pairs - j), "100:400"]
            f.write("\t".join(row) + "\n")
    return primers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=1e8)
    ap.add_argument("--row-len", type=int, default=1_000_000)
    ap.add_argument("--clusters", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--seedmms", type=int, default=1)
    ap.add_argument("--lookahead", type=int, default=4)
    ap.add_argument("--model-bases", type=int, default=1_000_000, help="0: skip the model")
    a = ap.parse_args()
    import torch  # noqa: F401  (one HIP runtime per process: torch's, as in the GPU suite)
    from multiprime_amd import maxset
    from multiprime_amd._abi import Library
    from multiprime_amd.synth import offtarget_case
    lib = Library()
    with tempfile.TemporaryDirectory() as td:
        n_rows = max(1, int(a.bases) // a.row_len)
        t0 = time.time()
        _, bg = offtarget_case(td, n_rows, a.row_len, 2, 3, n_degenerate=0)
        inp = os.path.join(td, "candidates.txt")
        primers = candidates(inp, a.clusters, a.pairs, 7)
        make_s = time.time() - t0
        base = ["-i", inp, "-o", os.path.join(td, "final.xls")]
        for label, extra in (("with -r", ["-r", bg, "--seedmms", str(a.seedmms), "--lookahead", str(a.lookahead)]), ("without -r", [])):
            opts = maxset.parse_args(base + extra)
            t0 = time.time()
            with contextlib.redirect_stdout(io.StringIO()):
                cover = maxset.run(opts, library=lib)
            rec = {"step": "run() " + label, "bases": n_rows * a.row_len, "clusters": a.clusters, "pairs_per_cluster": a.pairs,
                   "primers": len(set(primers)), "make_input_s": round(make_s, 2), "run_s": round(time.time() - t0, 3),
                   "selected_clusters": sum(1 for line in open(opts.out).read().splitlines()[1:] if line.split("\t")[1])}
            if cover.ot is not None:
                st = cover.ot.stats
                rec.update(seedmms=a.seedmms, lookahead=a.lookahead, adds=st["adds"], scan_ms=round(st["scan_ms"], 3), bin_ms=round(st["bin_ms"], 3),
                           join_ms=round(st["join_ms"], 3), pairs_with_products=len(cover.ot.pairs), tested_pairs=len(cover.ot_log),
                           rejected=sum(1 for r in cover.ot_log if r[6] == "rejected"),
                           first_add=dict(zip(("primers", "reads", "scan_ms", "bin_ms", "join_ms"), (round(x, 3) for x in st["per_add"][0]))),
                           later_adds_median=dict(zip(("primers", "reads", "scan_ms", "bin_ms", "join_ms"),
                                                      (round(float(np.median(x)), 3) for x in zip(*st["per_add"][1:])))) if st["adds"] > 1 else None,
                           later_adds_max=dict(zip(("primers", "reads", "scan_ms", "bin_ms", "join_ms"),
                                                   (round(float(np.max(x)), 3) for x in zip(*st["per_add"][1:])))) if st["adds"] > 1 else None)
                cover.ot.close()
            print(json.dumps(rec), flush=True)
        if a.model_bases:
            import setscreen_ref as ref
            from multiprime_amd.host import Fasta
            data, off = Fasta(bg).rows()
            piece = data[: a.model_bases].tobytes().decode()
            n_reads = sum(len(ref.reads_of(p, 12)) for p in set(primers))
            t0 = time.time()
            ref.sites([piece], primers[:1], 12, a.seedmms)
            wall = time.time() - t0
            print(json.dumps({"step": "model (tests/setscreen_ref.py, one core), sites of ONE read", "bases": len(piece), "wall_s": round(wall, 2),
                              "scaled_to": {"reads": n_reads, "bases": n_rows * a.row_len},
                              "scaled_s": round(wall * n_reads * n_rows * a.row_len / len(piece), 0),
                              "note": "scaled linearly by reads x bases from the sample; the join is not included"}), flush=True)


if __name__ == "__main__":
    main()
