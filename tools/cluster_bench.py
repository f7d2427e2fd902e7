#!/usr/bin/env python3
"""Clustering by identity at scale (mp_cluster_greedy): N seeded records of about 1 kb in planted families — a random root per family,
members with 0 .. 12 % substitutions and one deletion of 1..4 bases, a tenth of them exact duplicates of another member — at -c 0.8 and
-c 1 in alternating runs.  Per configuration: the call's time (median of the repeats), sequences per second, the clusters found, the
stage times and counts of mp_cluster_stats and the pair kernel's cell rate.  For scale only, the rate of the plain Python yardstick
(tests/cluster_ref.py) on one core of the same machine, on a small input of the same make.

    python tools/cluster_bench.py [--records 10000,100000,1000000] [--identities 800,1000] [--repeats 2] [--out profiles/cluster_scale.txt]
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


def make_chunk(rng, roots, n, length):
    letters = np.frombuffer(b"ACGT", np.uint8)
    mat = roots[rng.integers(0, len(roots), size=n)]
    rate = rng.choice(np.array([0.0, 0.01, 0.03, 0.06, 0.12], np.float32), size=n)
    sub = rng.random((n, length), dtype=np.float32) < rate[:, None]
    mat[sub] = letters[rng.integers(0, 4, size=int(sub.sum()))]
    p, g = rng.integers(50, length - 50, size=n), rng.integers(1, 5, size=n)
    dup = np.flatnonzero(rng.random(n) < 0.1)
    dup = dup[dup > 0]
    mat[dup], p[dup], g[dup] = mat[dup - 1], p[dup - 1], g[dup - 1]
    col = np.arange(length)[None, :]
    keep = (col < p[:, None]) | (col >= (p + g)[:, None])
    return mat[keep], keep.sum(axis=1)


def make_records(n, length, family, seed):
    """(data, off): n records in families of about `family` members, made in chunks of 50000."""
    rng = np.random.default_rng(seed)
    roots = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=((n + family - 1) // family, length))]
    parts = [make_chunk(rng, roots, min(50000, n - a), length) for a in range(0, n, 50000)]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.concatenate([x[1] for x in parts]), out=off[1:])
    return np.concatenate([x[0] for x in parts]), off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="10000,100000,1000000")
    ap.add_argument("--identities", default="800,1000")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--length", type=int, default=1000)
    ap.add_argument("--family", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from multiprime_amd._abi import Library
    import cluster_ref
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    idents = [int(x) for x in args.identities.split(",")]
    ctx = Library().context(0)
    say(f"clustering by identity: records of ~{args.length} bases in families of ~{args.family}, W = 32, min_votes 1; {args.repeats} alternating runs per identity")
    for n in (int(x) for x in args.records.split(",")):
        data, off = make_records(n, args.length, args.family, 2)
        ctx.cluster_load(data, off)
        times = {p: [] for p in idents}
        last = {}
        for rep in range(args.repeats + 1):                    # (the first round warms up: allocations, first launches)
            for p in idents:
                t0 = time.perf_counter()
                cluster_of, reps, _ = ctx.cluster_greedy(identity_permille=p)
                dt = time.perf_counter() - t0
                if rep or args.repeats == 0:
                    times[p].append(dt)
                    last[p] = (ctx.cluster_stats(), len(reps))
        for p in idents:
            (ms, counts), n_clusters = last[p]
            med = statistics.median(times[p])
            say(f"N={n} -c {p / 1000:g}: call {med * 1e3:.1f} ms (min {min(times[p]) * 1e3:.1f}, max {max(times[p]) * 1e3:.1f}), {n / med:.0f} sequences/s, "
                f"{n_clusters} clusters in {counts['rounds']} round(s); index {ms['index_ms']:.1f} ms, seed {ms['seed_ms']:.1f} ms, DP {ms['dp_ms']:.1f} ms, "
                f"host resolve {ms['resolve_ms']:.1f} ms; {counts['pairs']} candidate pairs, {counts['cells'] / 1e9:.2f} G cells, "
                f"{counts['cells'] / max(ms['dp_ms'], 1e-6) / 1e6:.2f} G cells/s in the pair kernel")
    ctx.close()
    # the yardstick on one core, for scale (it is not a competitor)
    data, off = make_records(60, 300, 10, 3)
    seqs = [data[off[i]:off[i + 1]].tobytes().decode() for i in range(60)]
    t0 = time.perf_counter()
    got = cluster_ref.cluster(seqs, identity_permille=800)
    dt = time.perf_counter() - t0
    say(f"yardstick (plain Python, one core, same machine): 60 records of ~300 bases, {len(got[1])} clusters, {60 / dt:.1f} sequences/s")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
