#!/usr/bin/env python3
"""The global-optimum selection (-m multiPrime2) on synthetic alignments (profiles/subset.txt): device time of the three kernels of
csrc/subset.hip (HIP events around each, mp_subset_timing) and the wall time of NN_degenerate.run() with method 2 — beside the same run
with method 1 — after a warm-up run, over several repetitions.

    python tools/subset_bench.py [--rows 131072 1048576 --cols 1000 -n 4 6 -v 1 --repeats 3 --dump FILE]        (needs the GPU)
    python tools/subset_bench.py --reference FILE --script PATH/multiPrime2-core_V2.py [--only-n 4 --limit 8]   (no GPU: one host core)

--dump writes a sample of the searched windows' tables (seed, cover items, cover_number; every --sample-every-th planned window) as JSON;
--reference times the reference's own get_Y_position (remove_elements inside it) on exactly those tables on one core and says how many
windows that was.  The reference script is imported by path and is not part of this repository."""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def run_once(path, out, method, n, v, k, dump=None, sample_every=50):
    from multiprime_amd import iupac, subset
    from multiprime_amd.core import NN_degenerate
    app = NN_degenerate(seq_file=path, primer_length=k, coverage=0.6, number_of_dege_bases=n, score_of_dege_bases=10, product_len=100,
                        position="1,2,-1", variation=v, raw_entropy_threshold=3.6, distance=4, GC="0.2,0.7", nproc=1, outfile=out,
                        write_json=False, method=method)
    try:
        t0 = time.time()
        app.run()
        wall = time.time() - t0
        stats = dict(app.stats)
        if dump is not None and method == "multiPrime2":
            # the tables of a sample of the planned windows, as the reference would see them (needs the ordered tables: a plan of its own)
            plan = app._plan(keep_tables=True)
            wins, s_window, s_seed, s_cover, _, _ = subset.plan_searches(plan)
            picked = set(wins.tolist()[::sample_every])
            for i, w in enumerate(s_window.tolist()):
                if w in picked:
                    codes, counts, _ = plan.window_table(w, 0)
                    dump.append({"window": w, "n": n, "v": v, "seed": "".join("ACGT"[b] for b in s_seed[i].tolist()),
                                 "cover": list(zip(iupac.strings_of(iupac.SYMBOL_LUT[codes]), counts.tolist())), "cover_number": int(s_cover[i])})
            plan.close()
    finally:
        app.ctx.close()
    return wall, stats


def bench(a):
    from multiprime_amd.synth import synth_block, to_fasta
    dump = [] if a.dump else None
    with tempfile.TemporaryDirectory() as td:
        for rows in a.rows:
            path = os.path.join(td, "synth_%d.fa" % rows)
            t0 = time.time()
            with open(path, "wb") as f:
                for r0 in range(0, rows, 65536):
                    f.write(to_fasta(synth_block(r0, min(65536, rows - r0), a.cols, a.seed), r0))
            print("# synth %d x %d (seed %d) written in %.1f s" % (rows, a.cols, a.seed, time.time() - t0), flush=True)
            out = os.path.join(td, "out.tsv")
            run_once(path, out, "multiPrime1", a.n[0], a.v, a.l)                       # warm-up: runtime, code objects, file cache
            for n in a.n:
                run_once(path, out, "multiPrime2", n, a.v, a.l)                        # warm-up of this shape
                for rep in range(a.repeats):
                    w1, s1 = run_once(path, out, "multiPrime1", n, a.v, a.l)
                    w2, s2 = run_once(path, out, "multiPrime2", n, a.v, a.l, dump if rep == 0 and rows == a.rows[0] else None, a.sample_every)
                    ms = s2["subset_kernel_ms"]
                    print("%d x %d -l %d -n %d -v %d rep %d: kernels records %.3f ms, step sets %.3f ms, search %.3f ms; searches %d (windows planned %d); "
                          "search call %.3f s; run() method 2 %.3f s (wall %.3f), method 1 %.3f s (wall %.3f); rows out %d / %d"
                          % (rows, a.cols, a.l, n, a.v, rep, ms[0], ms[1], ms[2], s2["subset_searches"], s2["windows_planned"], s2["subset_search_s"],
                             s2["run_s"], w2, s1["run_s"], w1, s2["n_rows"], s1["n_rows"]), flush=True)
    if a.dump:
        with open(a.dump, "w") as f:
            json.dump(dump, f)
        print("# %d searches of the first shape written to %s" % (len(dump), a.dump))


def reference(a):
    spec = importlib.util.spec_from_file_location("mpcore2_v2", a.script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    calls = json.load(open(a.reference))
    by = {}
    for c in calls:
        by.setdefault((c["n"], c["v"]), []).append(c)
    for (n, v), cs in sorted(by.items()):
        if a.only_n and n not in a.only_n:
            continue
        cs = cs[: a.limit] if a.limit else cs
        app = object.__new__(mod.NN_degenerate)
        app.number_of_dege_bases, app.variation = n, v
        t0 = time.process_time()
        for c in cs:
            cover = {u: m for u, m in c["cover"]}
            app.get_Y_position(c["seed"], set(cover), c["cover_number"], cover)
        dt = time.process_time() - t0
        print("reference get_Y_position, one core, -n %d -v %d: %d searches of %d windows (largest table %d k-mers): %.2f s, %.3f s per search"
              % (n, v, len(cs), len({c["window"] for c in cs}), max(len(c["cover"]) for c in cs), dt, dt / max(len(cs), 1)))


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, nargs="+", default=[131072, 1048576])
    p.add_argument("--cols", type=int, default=1000)
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("-l", type=int, default=18)
    p.add_argument("-n", type=int, nargs="+", default=[4, 6])
    p.add_argument("-v", type=int, default=1)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--dump", default=None)
    p.add_argument("--sample-every", type=int, default=50)
    p.add_argument("--reference", default=None)
    p.add_argument("--script", default=None)
    p.add_argument("--only-n", type=int, nargs="*", default=None, help="--reference: only these -n")
    p.add_argument("--limit", type=int, default=0, help="--reference: at most this many searches per setting")
    a = p.parse_args()
    if a.reference:
        reference(a)
    else:
        bench(a)
