#!/usr/bin/env python3
"""The read-to-primer assignment on a synthetic sequencing run (profiles/ont.txt): the device time of the assignment kernels
(mp_ont_stats, HIP events), the wall time of ONTprimer.run(), and beside them a one-core loop of the same difflib calls over a
subsample of the reads, scaled linearly to the whole run.  The loop's (key, rounded ratio) per read end must equal the device's.

    python tools/ont_bench.py [--reads 200000 --primers 96 --sample 200 --seed 3]     (needs the GPU)

The run: --primers primers of 18 .. 22 bases in pairs, about two thirds of them with one to three two- or three-fold degenerate
positions (about 1000 keys after expansion and reverse complement); a read is an amplicon of a pair with 100 .. 400 bases between
the primers, on either strand, each end with 0 .. 3 substitutions or one-base indels; 2 % of the reads are unrelated.  Plain FASTQ."""
import argparse
import difflib
import os
import random
import sys
import tempfile
import time


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from multiprime_amd import ontprimer as op  # noqa: E402
from multiprime_amd._abi import Library  # noqa: E402

COMPLEMENT = str.maketrans("ACGT", "TGCA")


def dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def damage(rng, s, n):
    s = list(s)
    for _ in range(n):
        at = rng.randrange(len(s))
        kind = rng.random()
        if kind < 0.5:
            s[at] = rng.choice("ACGT")
        elif kind < 0.75:
            del s[at]
        else:
            s.insert(at, rng.choice("ACGT"))
    return "".join(s)


def make_panel(rng, n):
    out = []
    for i in range(n):
        s = list(dna(rng, rng.randint(18, 22)))
        if i % 3:
            for at in rng.sample(range(len(s)), rng.randint(1, 3)):
                s[at] = rng.choice([c for c in "RYMKSWHBVD" if s[at] in op.DEGENERATE[c]])
        out.append((">p%d_%s" % (i // 2, "FR"[i % 2]), "".join(s)))
    return out


def make_reads(rng, panel, n):
    expansions = [op.expand(s) for _, s in panel]
    reads = []
    for _ in range(n):
        if rng.random() < 0.02:
            reads.append(dna(rng, rng.randint(150, 450)))
            continue
        pair = rng.randrange(len(panel) // 2)
        f, r = rng.choice(expansions[2 * pair]), rng.choice(expansions[2 * pair + 1])
        amp = damage(rng, f, rng.randint(0, 3)) + dna(rng, rng.randint(100, 400)) + damage(rng, r, rng.randint(0, 3)).translate(COMPLEMENT)[::-1]
        reads.append(amp.translate(COMPLEMENT)[::-1] if rng.random() < 0.5 else amp)
    return reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200000)
    ap.add_argument("--primers", type=int, default=96)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--length", type=int, default=18)
    ap.add_argument("--min-ident", type=float, default=0.6)
    a = ap.parse_args()
    rng = random.Random(a.seed)
    panel = make_panel(rng, a.primers)
    reads = make_reads(rng, panel, a.reads)
    lib = Library()
    with tempfile.TemporaryDirectory() as td:
        primers, fq = os.path.join(td, "panel.fasta"), os.path.join(td, "reads.fq")
        with open(primers, "w") as f:
            f.write("".join("%s\n%s\n" % p for p in panel))
        with open(fq, "w") as f:
            f.write("".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
        walls, devs = [], []
        for _ in range(3):                             # the first run pays the context and the first launch
            app = op.ONTprimer(fq, primers, outfile=os.path.join(td, "out"), primer_len=a.length, min_ident=a.min_ident, library=lib)
            t0 = time.time()
            tally = app.run()
            walls.append(time.time() - t0)
            devs.append(app.stats[0]["assign_ms"])
        keys = app.keys
        n_pairs = 2 * a.reads * len(keys)
        print("reads %d, primers %d, keys %d, pieces %d, comparisons %.3g" % (a.reads, a.primers, len(keys), 2 * a.reads, n_pairs))
        print("device (HIP events, mp_ont_stats), three runs: %s ms" % ", ".join("%.1f" % d for d in devs))
        print("run() wall, three runs: %s s" % ", ".join("%.2f" % w for w in walls))
        print("pairs in the .num file: %d, reads with NA at an end: %d" % (len(tally.counts), sum(c for p, c in tally.counts.items() if "NA" in p.split("\t"))))
        # the same calls on one core over a subsample, and the device's answers for it
        sample = [p for b in op.read_pieces(fq, "fq", a.length, a.sample) for p in b][:2 * a.sample]
        t0 = time.time()
        cpu = []
        for piece in sample:
            ratios = [round(difflib.SequenceMatcher(None, piece, k).ratio(), 2) for k in keys]
            top = max(ratios)
            cpu.append((ratios.index(top), top))
        cpu_s = time.time() - t0
        ctx = lib.context(0)
        try:
            ctx.ont_set_keys(*op.pack(keys))
            lens, key, m = app.assign(ctx, sample, op.rank_table())
        finally:
            ctx.close()
        ratios = op.ratio_table()
        dev = [(int(k), float(ratios[int(n) + len(keys[int(k)]), int(x)])) for n, k, x in zip(lens, key, m)]
        assert dev == cpu, "the device's assignments differ from difflib's on the subsample"
        scaled = cpu_s * a.reads / a.sample
        dev_s, wall = min(devs) / 1e3, min(walls)
        print("difflib on one core, %d reads: %.2f s (%.1f us per comparison); scaled linearly to %d reads: %.0f s" % (
            a.sample, cpu_s, 1e6 * cpu_s / (len(sample) * len(keys)), a.reads, scaled))
        print("the subsample's %d assignments equal the device's" % len(sample))
        print("ratio: %.0f x against the device time (best of three), %.0f x against run() wall (best of three)" % (scaled / dev_s, scaled / wall))


if __name__ == "__main__":
    main()
