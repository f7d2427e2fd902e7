#!/usr/bin/env python3
"""The star alignment at scale (mp_star_round): the reference workflow's own 500-record cluster through StarAlignment.run(), then
synthetic families of N records of about 1 kb — one random root, members with 0 .. 6 % substitutions and one deletion of 1..4 bases —
two rounds at W = 32 in repeated runs.  Per size and round: the call's time (median of the repeats), the stage times of mp_star_stats,
the ratio to anchored alignment's own pass over 10^6 queries of 1 kb (profiles/anchor_scale.txt: 365 ms, scaled to N), and for the
kernels this change adds the bytes they move against their time.

    python tools/star_bench.py [--records 10000,100000,1000000] [--repeats 2] [--out profiles/star_scale.txt]
"""
import argparse
import gzip
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ANCHOR_PASS_MS_PER_RECORD = 365.0 / 1e6         # profiles/anchor_scale.txt: 10^6 queries of 1 kb at W = 32
STAGES = ("vote_ms", "dp_ms", "trace_ms", "profile_ms", "write_ms", "count_ms", "readback_ms", "call_ms")


def make_family(n, length, seed):
    """(data, off): record 0 is the root (the longest), the others its mutated copies, made in chunks of 50000."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    root = letters[rng.integers(0, 4, size=length)]
    parts, lens = [root], [np.array([length])]
    for a in range(1, n, 50000):
        k = min(50000, n - a)
        mat = np.repeat(root[None, :], k, axis=0)
        rate = rng.choice(np.array([0.0, 0.01, 0.03, 0.06], np.float32), size=k)
        sub = rng.random((k, length), dtype=np.float32) < rate[:, None]
        mat[sub] = letters[rng.integers(0, 4, size=int(sub.sum()))]
        p, g = rng.integers(50, length - 50, size=k), rng.integers(1, 5, size=k)
        col = np.arange(length)[None, :]
        keep = (col < p[:, None]) | (col >= (p + g)[:, None])
        parts.append(mat[keep])
        lens.append(keep.sum(axis=1))
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.concatenate(lens), out=off[1:])
    return np.concatenate(parts), off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="10000,100000,1000000")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-cluster", action="store_true", help="skip the 500-record cluster")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from multiprime_amd._abi import Library
    from multiprime_amd.starmsa import StarAlignment, anchor_of_counts
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = Library()
    if not args.no_cluster:
        with tempfile.TemporaryDirectory() as td:
            inp, out = os.path.join(td, "Cluster_0_20727.tfa"), os.path.join(td, "Cluster_0_20727.tmsa")
            with open(inp, "wb") as f:
                f.write(gzip.open(os.path.join(REPO, "tests", "golden", "inputs", "Cluster_0_20727.tfa.gz")).read())
            runs = []
            for _ in range(args.repeats + 1):                  # (the first run warms up)
                t0 = time.perf_counter()
                app = StarAlignment(inp, out, rounds=args.rounds, library=lib).run()
                runs.append(time.perf_counter() - t0)
            say(f"Cluster_0_20727 (500 records of 1698..1867 bases), {len(app.anchors())} round(s): run() {statistics.median(runs[1:]) * 1e3:.1f} ms "
                f"(load {app.stats['load_s'] * 1e3:.1f}, align {app.stats['align_s'] * 1e3:.1f}, write {app.stats['write_s'] * 1e3:.1f}), width {app.width}")
            for k, st in enumerate(app.round_stats):
                say(f"  round {k}: n {st['n']} width {st['width']} placed {st['placed']} realigned {st['realigned']}; " +
                    ", ".join(f"{s[:-3]} {st[s]:.2f}" for s in STAGES) + f" ms; {st['cells'] / 1e6:.1f} M cells")
    ctx = lib.context(0)
    say(f"synthetic families: records of ~{args.length} bases, W = 32, {args.rounds} rounds, {args.repeats} timed runs after one warm-up")
    for n in (int(x) for x in args.records.split(",")):
        data, off = make_family(n, args.length, 2)
        ctx.star_load(data, off)
        per_round = {}
        for rep in range(args.repeats + 1):
            anchor = data[off[0]:off[1]].tobytes()
            for k in range(args.rounds):
                t0 = time.perf_counter()
                meta, ins, width = ctx.star_round(anchor)
                dt = time.perf_counter() - t0
                ms, counts = ctx.star_stats()
                if rep or args.repeats == 0:
                    per_round.setdefault(k, []).append((dt, ms, counts, width, len(anchor)))
                if k + 1 < args.rounds:
                    anchor = anchor_of_counts(ctx.star_counts(), counts["placed"])
        for k, runs in per_round.items():
            med = statistics.median(r[0] for r in runs)
            _, ms, counts, width, n_anchor = runs[-1]
            base = ANCHOR_PASS_MS_PER_RECORD * n
            slots = (n_anchor + 8) & ~7
            moved = {"profile": 2.0 * n * slots, "write": float(n) * (width + n_anchor), "count": float(n) * width}
            say(f"N={n} round {k}: call {med * 1e3:.1f} ms = {med * 1e3 / base:.2f} x the anchored pass ({base:.1f} ms); n {n_anchor} width {width} placed "
                f"{counts['placed']} realigned {counts['realigned']} batches {counts['batches']}; " + ", ".join(f"{s[:-3]} {ms[s]:.2f}" for s in STAGES) +
                f" ms; {counts['cells'] / max(ms['dp_ms'], 1e-6) / 1e6:.1f} G cells/s in the sweep; new kernels: " +
                ", ".join(f"{what} {b / 1e9:.2f} GB at {b / max(ms[what + '_ms'], 1e-6) / 1e6:.0f} GB/s" for what, b in moved.items()))
        ctx.star_free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
