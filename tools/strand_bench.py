#!/usr/bin/env python3
"""What both strands cost (profiles/strands.txt): the three unaligned-sequence stages on the synthetic sets of their own benchmarks
(tools/anchor_bench.py, tools/star_bench.py and its 500-record cluster, tools/cluster_bench.py) with every second record replaced by its
reverse complement, the switch off and on in alternating runs.  Per stage: the call's time (median of the repeats) off and on, their
ratio, the stage times the library reports, and the vote kernel's share of the device time.  With the switch off the mixed set is
merely a harder input (half of it unrelated on the forward strand); the plain set, switch off, is what the stage's own benchmark times.

    python tools/strand_bench.py [--queries 100000 --records 100000 --cluster-records 20000 --repeats 3 --out profiles/strands.txt]
"""
import argparse
import gzip
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCATGCA"):
    _COMP[_a] = _b


def turn_every_second(data, off):
    """The records with the odd-numbered ones reversed and complemented."""
    out = data.copy()
    for q in range(1, len(off) - 1, 2):
        out[off[q]:off[q + 1]] = _COMP[data[off[q]:off[q + 1]][::-1]]
    return out


def timed(fn, repeats):
    """Median wall time of fn() over `repeats` runs after one warm-up, and the last result."""
    times, res = [], None
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        res = fn()
        if rep:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--cluster-records", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from anchor_bench import make_queries
    from cluster_bench import make_records
    from star_bench import make_family
    from multiprime_amd._abi import ANCHOR_REVERSED, Library
    from multiprime_amd.msa import parse_records
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    lib = Library()
    ctx = lib.context(0)
    say(f"both strands: every second record turned; {args.repeats} timed runs after one warm-up, median; single-box numbers")

    # anchored alignment
    anchor = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(1).integers(0, 4, size=1000)]
    data, off = make_queries(anchor, args.queries, 2)
    mixed = turn_every_second(data, off)
    ctx.anchor_set(anchor, np.arange(1000), 1000, band=32)
    res = {}
    for name, both, d in (("plain set, off", False, data), ("mixed set, off", False, mixed), ("mixed set, on", True, mixed)):
        ctx.anchor_strands(both)
        med, (_, meta, _) = timed(lambda: ctx.anchor_align(d, off), args.repeats)
        ms, _ = ctx.anchor_stats()
        res[name] = med
        dev = ms["vote_ms"] + ms["dp_ms"] + ms["trace_ms"]
        say(f"anchor N={args.queries} W=32 {name}: call {med * 1e3:.1f} ms; vote {ms['vote_ms']:.2f} ms ({100 * ms['vote_ms'] / dev:.1f} % of the device time), "
            f"DP {ms['dp_ms']:.1f} ms, traceback+emit {ms['trace_ms']:.1f} ms; turned {int((meta[:, 7] & ANCHOR_REVERSED != 0).sum())}, rejected {int((meta[:, 7] & 1).sum())}")
    say(f"anchor: on / off on the mixed set {res['mixed set, on'] / res['mixed set, off']:.3f}, on (mixed) / off (plain) {res['mixed set, on'] / res['plain set, off']:.3f}")
    ctx.anchor_strands(False)

    # star alignment: the synthetic family, then the workflow's 500-record cluster
    sets = []
    data, off = make_family(args.records, 1000, 2)
    sets.append((f"family N={args.records}", data, off))
    _, cdata, coff = parse_records(gzip.open(os.path.join(REPO, "tests", "golden", "inputs", "Cluster_0_20727.tfa.gz")).read())
    keep = (cdata[: coff[-1]] != ord("-")) & (cdata[: coff[-1]] != ord("."))
    kept = np.zeros(len(keep) + 1, np.int64)
    np.cumsum(keep, out=kept[1:])
    sets.append(("Cluster_0_20727 (500 records)", np.ascontiguousarray(cdata[: coff[-1]][keep]), kept[coff]))
    for label, data, off in sets:
        mixed = turn_every_second(data, off)
        centre = int(np.argmax(np.diff(off)))
        centre -= centre % 2                                    # (an even record: as given in both sets)
        anchor = data[off[centre]:off[centre + 1]].tobytes().upper()
        res = {}
        for name, both, d in (("plain set, off", False, data), ("mixed set, off", False, mixed), ("mixed set, on", True, mixed)):
            ctx.anchor_strands(both)

            def one_round():
                ctx.star_load(d, off)                           # (a turned record stays turned: every run starts from the records as given)
                t0 = time.perf_counter()
                out = ctx.star_round(anchor)
                return time.perf_counter() - t0, out
            runs = [one_round() for _ in range(args.repeats + 1)][1:]
            med, meta = statistics.median(r[0] for r in runs), runs[-1][1][0]
            ms, counts = ctx.star_stats()
            res[name] = med
            dev = sum(ms[k] for k in ("vote_ms", "dp_ms", "trace_ms", "profile_ms", "write_ms", "count_ms"))
            say(f"star {label} round 0 {name}: call {med * 1e3:.1f} ms; vote {ms['vote_ms']:.2f} ms ({100 * ms['vote_ms'] / dev:.1f} % of the device time), "
                f"DP {ms['dp_ms']:.1f} ms, traceback {ms['trace_ms']:.1f} ms; placed {counts['placed']} realigned {counts['realigned']} "
                f"turned {int((meta[:, 7] & ANCHOR_REVERSED != 0).sum())}")
        say(f"star {label}: on / off on the mixed set {res['mixed set, on'] / res['mixed set, off']:.3f}, on (mixed) / off (plain) {res['mixed set, on'] / res['plain set, off']:.3f}")
        ctx.star_free()
    ctx.anchor_strands(False)

    # clustering
    data, off = make_records(args.cluster_records, 1000, 50, 2)
    mixed = turn_every_second(data, off)
    res = {}
    for name, both, d in (("plain set, forward call", False, data), ("mixed set, forward call", False, mixed), ("mixed set, both strands", True, mixed)):
        ctx.cluster_load(d, off)
        med, out = timed((lambda: ctx.cluster_greedy_strands(identity_permille=800)) if both else (lambda: ctx.cluster_greedy(identity_permille=800)), args.repeats)
        ms, counts = ctx.cluster_stats()
        res[name] = med
        dev = ms["index_ms"] + ms["seed_ms"] + ms["dp_ms"]
        say(f"cluster N={args.cluster_records} -c 0.8 {name}: call {med * 1e3:.1f} ms; {len(out[1])} clusters in {counts['rounds']} round(s); index {ms['index_ms']:.1f} ms, "
            f"seed (count + vote) {ms['seed_ms']:.1f} ms ({100 * ms['seed_ms'] / dev:.1f} % of the device time), DP {ms['dp_ms']:.1f} ms, host resolve {ms['resolve_ms']:.1f} ms; "
            f"{counts['pairs']} pairs aligned" + (f", {int(out[3].sum())} members on the minus strand" if both else ""))
    say(f"cluster: both strands (mixed) / forward call (plain) {res['mixed set, both strands'] / res['plain set, forward call']:.3f}; "
        f"both strands / forward call on the mixed set {res['mixed set, both strands'] / res['mixed set, forward call']:.3f} (the forward call leaves the turned half in clusters of its own)")
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
