#!/usr/bin/env python3
"""Anchored alignment at scale (mp_anchor_align): N seeded queries of about 1 kb — the anchor with 2 % substitutions and one deletion
of 1..4 bases each — against a 1 kb anchor, at W = 32 and W = 128 in alternating runs.  Per configuration: the call's time (median of
the repeats), cell updates per second, and the split into vote, DP, traceback + emit and read-back that mp_anchor_stats reports.  For
scale only, the cell rate of the plain Python yardstick (tests/anchor_ref.py) on one core of the same machine.

    python tools/anchor_bench.py [--queries 100000,1000000] [--bands 32,128] [--repeats 3] [--out profiles/anchor_scale.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def make_queries(anchor, n, seed):
    rng = np.random.default_rng(seed)
    L = len(anchor)
    mat = np.broadcast_to(anchor, (n, L)).copy()
    sub = rng.random((n, L)) < 0.02
    mat[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(sub.sum()))]
    p, g = rng.integers(50, L - 50, size=n), rng.integers(1, 5, size=n)
    col = np.arange(L)[None, :]
    keep = (col < p[:, None]) | (col >= (p + g)[:, None])
    off = np.zeros(n + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=off[1:])
    return mat[keep], off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", default="100000,1000000")
    ap.add_argument("--bands", default="32,128")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from multiprime_amd._abi import Library
    import anchor_ref
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    anchor = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(1).integers(0, 4, size=args.length)]
    bands = [int(x) for x in args.bands.split(",")]
    ctx = Library().context(0)
    say(f"anchored alignment: anchor {args.length}, queries = anchor with 2 % substitutions and one 1..4-base deletion; {args.repeats} alternating runs per band")
    for n in (int(x) for x in args.queries.split(",")):
        data, off = make_queries(anchor, n, 2)
        times = {W: [] for W in bands}
        last = {}
        for rep in range(args.repeats + 1):                    # (the first round warms up: allocations, first launches)
            for W in bands:
                ctx.anchor_set(anchor, np.arange(args.length), args.length, band=W)
                t0 = time.perf_counter()
                rows, meta, _ = ctx.anchor_align(data, off)
                dt = time.perf_counter() - t0
                if rep:
                    times[W].append(dt)
                    last[W] = (ctx.anchor_stats(), int((meta[:, 7] & 1).sum()), int((meta[:, 7] & 2 != 0).sum()), int(meta[:, 4].sum()))
        for W in bands:
            (ms, counts), rejected, warned, n_del = last[W]
            med = statistics.median(times[W])
            say(f"N={n} W={W}: call {med * 1e3:.1f} ms (min {min(times[W]) * 1e3:.1f}, max {max(times[W]) * 1e3:.1f}), "
                f"{counts['cells'] / med / 1e9:.2f} G cells/s over the call, {counts['cells'] / (ms['dp_ms'] * 1e-3) / 1e9:.2f} G cells/s in the DP kernel; "
                f"vote {ms['vote_ms']:.1f} ms, DP {ms['dp_ms']:.1f} ms, traceback+emit {ms['trace_ms']:.1f} ms, read-back {ms['readback_ms']:.1f} ms; "
                f"{counts['batches']} batch(es), traceback bits {counts['traceback_bytes'] / 2 ** 30:.2f} GiB; rejected {rejected}, band warnings {warned}, "
                f"deleted columns {n_del}")
    ctx.close()
    # the yardstick on one core, for scale (it is not a competitor)
    data, off = make_queries(anchor[:300], 4, 3)
    a = anchor[:300].tobytes().decode()
    t0 = time.perf_counter()
    cells = 0
    for q in range(4):
        s = data[off[q]:off[q + 1]].tobytes().decode()
        anchor_ref.align(s, a, list(range(300)), 300, band=32)
        cells += len(s) * 65
    dt = time.perf_counter() - t0
    say(f"yardstick (plain Python, one core, same machine): {cells / dt / 1e6:.2f} M cells/s")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
