#!/usr/bin/env python3
"""The identity merge on a synthetic cluster set (profiles/ani_merge.txt): what mp_ani_stats says for the device pass, and the
yardstick's table of mean ani_ppm against the planted substitution rate.

    python tools/ani_bench.py run   [--clusters 2000 --rare 1500 --seed 7 --sketch-size 1024]     (needs the GPU)
    python tools/ani_bench.py strands [the flags of run]                                         (needs the GPU; profiles/strands.txt)
    python tools/ani_bench.py table [--seeds 1 2 3 4 5]                                          (host only)

`run`: `--clusters` clusters, `--rare` of them with 1 .. 20 members, the others with 21 .. 500; a cluster is a root of 1 .. 10 kb
(synth_root) and members at 0 .. 3 % substitutions of it; half of the rare clusters' roots are a large cluster's root at 10 % (they
merge at -a 0.8), the others unrelated (they are compared with every larger cluster).  The records go to the device pass of
multiprime_amd/animerge.py (-t 20, -a 0.8, floor 0.7) without touching a file.
`strands`: the set of `run` with every second rare cluster turned (all its records reverse-complemented), through the device pass twice:
forward (`merge_clstr()` as `run` does) and with `both_strands=True` — sketch ms of both forms on the same records, compare ms, the
strand pass, and the merges with and without the flag.
`table`: per seed a 2 kb root and one copy at each rate; the pair's ani_ppm from tests/ani_ref.py at s = 1024 and 128."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from multiprime_amd.synth import synth_root  # noqa: E402

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def mutate(rng, root, rate):
    out = root.copy()
    hit = np.flatnonzero(rng.random(len(root)) < rate)
    out[hit] = (out[hit] + rng.integers(1, 4, size=len(hit), dtype=np.uint8)) & 3
    return out


def run(args, turn=False):
    from multiprime_amd.animerge import merge_clstr
    rng = np.random.default_rng(args.seed)
    n_large = args.clusters - args.rare
    sizes = np.concatenate([rng.integers(21, 501, size=n_large), rng.integers(1, 21, size=args.rare)])
    roots = [synth_root(int(rng.integers(1000, 10001)), args.seed * 100003 + k) for k in range(n_large)]
    for k in range(args.rare):
        roots.append(mutate(rng, roots[int(rng.integers(0, n_large))], 0.10) if k % 2 == 0 else synth_root(int(rng.integers(1000, 10001)), args.seed * 100003 + n_large + k))
    order = np.argsort(-sizes, kind="stable")
    chunks, lens, group_off = [], [], [0]
    for k in order.tolist():
        flip = turn and k >= n_large and (k - n_large) % 4 < 2       # half of the rare clusters: every second related one, every second unrelated one
        for m in range(int(sizes[k])):
            codes = mutate(rng, roots[k], rng.random() * 0.03) if m else roots[k]
            chunks.append(_ACGT[(3 - codes)[::-1] if flip else codes])
            lens.append(len(roots[k]))
        group_off.append(len(lens))
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    data = np.concatenate(chunks)
    print("clusters %d (rare %d%s), records %d, bases %d, s = %d" % (args.clusters, args.rare, ", every second one turned" if turn else "", len(lens),
                                                                   int(off[-1]), args.sketch_size))
    for both in ((False, True) if turn else (False,)):
        app = merge_clstr(threshold=20, ani=0.8, report_floor=0.7, sketch_size=args.sketch_size, both_strands=both,
                          clusters=[("c%d" % k, int(sizes[k])) for k in order.tolist()])
        app.load_records(data, off, group_off)
        t0 = time.time()
        numbers = app.compare()
        wall = time.time() - t0
        merged = sum(len(v) for v in app.decide(numbers).values())
        st = app.stats
        if turn:
            print("--both-strands (canonical sketches):" if both else "forward (no flag):")
        print("cluster pairs evaluated %d, rare clusters merged %d" % (len(numbers), merged))
        print("sketch_ms %.2f  compare_ms %.2f  sequence pairs %d  pairs/s %.3e  (device pass wall %.2f s)" % (
            st["sketch_ms"], st["compare_ms"], st["pairs"], st["pairs"] / max(st["compare_ms"], 1e-9) * 1e3, wall))
        if both:
            print("strand_ms %.2f (the mp_ani_groups_strand call over the %d decided merges, host wall)  merges on the other strand %d" % (
                st["strand_ms"], merged, st["n_minus"]))


def table(args):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import ani_ref as ref
    rates = (0.02, 0.05, 0.10, 0.15, 0.20)
    print("mean ani_ppm / 1e6 of a 2 kb root against its copy at a planted substitution rate, seeds %s" % args.seeds)
    print("rate      " + "  ".join("%5.2f" % r for r in rates) + "  unrelated")
    for s in (1024, 128):
        cols = []
        for rate in rates + (None,):
            got = []
            for seed in args.seeds:
                rng = np.random.default_rng([seed, 17])
                root = synth_root(2000, seed)
                other = synth_root(2000, seed + 1000) if rate is None else root.copy()
                if rate is not None:
                    hit = rng.choice(2000, size=int(rate * 2000), replace=False)
                    other[hit] = (other[hit] + rng.integers(1, 4, size=len(hit), dtype=np.uint8)) & 3
                a, b = (_ACGT[x].tobytes().decode() for x in (root, other))
                got.append(ref.pair(ref.sketch(a, s), ref.sketch(b, s), s)[2])
            cols.append(sum(got) / len(got) / 1e6)
        print("s = %-5d " % s + "  ".join("%5.3f" % c for c in cols[:-1]) + "  %5.3f" % cols[-1])


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    sub = p.add_subparsers(dest="cmd", required=True)
    for name in ("run", "strands"):
        r = sub.add_parser(name)
        r.add_argument("--clusters", type=int, default=2000)
        r.add_argument("--rare", type=int, default=1500)
        r.add_argument("--seed", type=int, default=7)
        r.add_argument("--sketch-size", type=int, default=1024)
    t = sub.add_parser("table")
    t.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3, 4, 5])
    a = p.parse_args()
    run(a, turn=a.cmd == "strands") if a.cmd in ("run", "strands") else table(a)
