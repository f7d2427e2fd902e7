"""Rules 7 and 8 of the reference's second workflow (multi-DegePrime.py) without Perl: trimming an alignment for DegePrime
(DEGEPRIME-1.1.0/TrimAlignment.pl, here on the host with numpy: a column count) and DegePrime itself (run_dege.py, which calls
DEGEPRIME-1.1.0/DegePrime.pl; here csrc/dege.hip on the GPU — the rule is stated in include/mprime_dege.h and INTEGRATION.md).

    python scripts/TrimAlignment.py -i cluster.msa -o cluster.trim.msa -min 0.9
    python scripts/run_dege.py -i cluster.trim.msa -o cluster.dege.out -l 18 -d 12

The trimmed alignment is byte-identical to the Perl script's.  The table has the Perl script's header and columns; Pos, NumberSpanning,
UniqueMers and Entropy are DegePrime's own numbers, the oligomer of a window comes from the deterministic restatement of its weighted
randomised merging (--seed picks the draws).  Every failure that makes the Perl scripts die, and every option this tool does not
serve, ends with exit status 2 and one sentence on stderr.
"""
from __future__ import annotations

import argparse
import os
import re
import sys
import time

import numpy as np

from ._abi import DEGE_MAX_ITERS, DEGE_MAX_L, DEGE_MIN_L, Library, MprimeError

HEADER = "Pos\tNumberSpanning\tUniqueMers\tEntropy\tPrimerDeg\tPrimerSeq\tNumberMatching\tFractionMatching"
# IUPAC letter of a set of bases: bit 0 = A, 1 = C, 2 = G, 3 = T (index 0: the empty set, never printed)
SET_LETTER = "?ACMGRSVTWYHKDBN"


class DegeError(Exception):
    """A failure that ends a command with status 2 and this sentence."""


def read_records(path):
    """[(id, sequence)] the way both Perl scripts read a FASTA file: the id is the first field of the '>' line split at white space, the
    lines of a record are joined as they are (without their line feed)."""
    out = []
    with open(path, "rb") as f:
        for line in f.read().decode("latin-1").split("\n"):
            if line.startswith(">"):
                out.append([re.split(r"\s+", line[1:])[0], []])
            elif out:
                out[-1][1].append(line)
    return [(i, "".join(s)) for i, s in out]


def valid_degeneracy(d: int) -> int:
    """DegePrime lowers -d to the largest value <= d of the form 2^a 3^b."""
    def ok(x):
        while x % 2 == 0:
            x //= 2
        while x % 3 == 0:
            x //= 3
        return x == 1
    if d < 1:
        raise DegeError(f"the maximum degeneracy must be a positive integer, not {d}")
    while not ok(d):
        d -= 1
    return d


def fmt(x: float) -> str:
    """Perl's stringification of a number: %.15g, never -0."""
    s = "%.15g" % x
    return "0" if s == "-0" else s


# ---- TrimAlignment ---------------------------------------------------------------------------------------------------------------------------
def _matrix(records, what):
    rows = [re.sub(r"\s+", "", s) for _, s in records]
    if len({len(r) for r in rows}) > 1:
        raise DegeError(f"{what}: the aligned sequences have different lengths")
    width = len(rows[0]) if rows else 0
    return np.frombuffer("".join(rows).encode("latin-1"), np.uint8).reshape(len(rows), width)


def kept_columns(records, cutoff=0.0, max_trailing=1.0, trailgap=False, ref=None):
    """The columns TrimAlignment.pl keeps (ascending) and the byte matrix of the records it prints."""
    # a record without sequence lines is passed over, unless it is the last one (the Perl loops)
    records = [r for k, r in enumerate(records) if r[1] != "" or k == len(records) - 1]
    if not records:
        raise DegeError("the alignment holds no sequence")
    m = _matrix(records, "TrimAlignment")
    if ref is not None:
        hit = [k for k, (i, _) in enumerate(records) if i == ref]
        if not hit:
            raise DegeError(f"the reference sequence {ref!r} was not found (only the part of an id before the first space counts)")
        row = m[hit[0]]
        cols = np.flatnonzero(((row >= 65) & (row <= 90)) | ((row >= 97) & (row <= 122)))
    else:
        total = len(records)
        c = m.copy()
        if trailgap:
            c[c == ord(".")] = ord("-")
        counts = (c != ord("-")).sum(axis=0)
        trailing = (c == ord(".")).sum(axis=0)
        used = np.flatnonzero(counts)
        n_cols = int(used[-1]) + 1 if len(used) else 0          # Perl's @counts ends at the last column anything but '-' was seen in
        cols = []
        for i in range(n_cols):
            if trailing[i] / total <= max_trailing:
                if total == trailing[i]:
                    raise DegeError(f"column {i} holds nothing but '.': its occupancy is a division by zero")
                if (counts[i] - trailing[i]) / (total - trailing[i]) >= cutoff:
                    cols.append(i)
        cols = np.array(cols, np.int64)
    if len(cols) == 0:
        raise DegeError("no column of the alignment is kept")
    return cols, records, m


def trim_alignment(records, cutoff=0.0, max_trailing=1.0, trailgap=False, ref=None) -> str:
    """The text TrimAlignment.pl writes: upper case, U -> T, the kept columns, and a letter in lower case where columns between it and the
    next kept column were removed in which the row has a base (columns removed after the last kept one mark nothing)."""
    cols, records, m = kept_columns(records, cutoff, max_trailing, trailgap, ref)
    up = m.copy()
    low = (up >= 97) & (up <= 122)
    up[low] -= 32
    up[up == ord("U")] = ord("T")
    word = ((up >= 65) & (up <= 90)) | ((up >= 48) & (up <= 57)) | (up == ord("_"))            # Perl's \w after the upper-casing
    run = np.zeros((up.shape[0], up.shape[1] + 1), np.int64)
    np.cumsum(word, axis=1, out=run[:, 1:])
    out = up[:, cols].copy()
    if len(cols) > 1:
        marked = (run[:, cols[1:]] - run[:, cols[:-1] + 1]) > 0
        body = out[:, :-1]
        letter = (body >= 65) & (body <= 90)
        body[marked & letter] += 32
    return "".join(">%s\n%s\n" % (i, row.tobytes().decode("latin-1")) for (i, _), row in zip(records, out))


def _parser(prog, doc):
    return argparse.ArgumentParser(prog=prog, description=doc, allow_abbrev=False)


def trim_main(argv=None):
    p = _parser("TrimAlignment.py", "Trim and format an alignment for run_dege.py (TrimAlignment.pl's flags)")
    p.add_argument("-i", dest="input", required=True, help="alignment (FASTA)")
    p.add_argument("-o", dest="out", required=True, help="output file")
    p.add_argument("-min", "--min", dest="cutoff", type=float, default=None, help="minimum occupancy of a kept column, 0..1 (default 0)")
    p.add_argument("-max_trailing", "--max_trailing", dest="max_trailing", type=float, default=1.0,
                   help="largest fraction of '.' in a kept column (default 1)")
    p.add_argument("-trailgap", "--trailgap", dest="trailgap", action="store_true", help="count '.' as '-'")
    p.add_argument("-ref", "--ref", dest="ref", default=None, help="keep the columns in which this sequence has a letter")
    a = p.parse_args(argv)
    try:
        if a.cutoff and not 0 <= a.cutoff <= 1:
            raise DegeError("allowed minimum occupancy (-min) range: 0 to 1")
        if a.cutoff and a.ref:
            raise DegeError("not possible to specify both minimum occupancy and reference sequence")
        text = trim_alignment(read_records(a.input), a.cutoff or 0.0, a.max_trailing, a.trailgap, a.ref or None)
    except DegeError as e:
        print(f"TrimAlignment.py: {e}", file=sys.stderr)
        sys.exit(2)
    with open(a.out, "w", encoding="latin-1", newline="") as f:
        f.write(text)


# ---- DegePrime -------------------------------------------------------------------------------------------------------------------------------
def read_trimmed(path):
    """The rows of a trimmed alignment as a byte matrix.  DegePrime.pl keeps its sequences in a hash: of two records with one id the later
    one stays."""
    by_id = {}
    for i, s in read_records(path):
        by_id[i] = s
    rows = list(by_id.values())
    if not rows:
        raise DegeError(f"{path} holds no sequence")
    if len({len(r) for r in rows}) > 1:
        raise DegeError("not all aligned sequences have the same length")
    if len(rows[0]) == 0:
        raise DegeError("the aligned sequences are empty")
    return np.frombuffer("".join(rows).encode("latin-1"), np.uint8).reshape(len(rows), len(rows[0]))


def table_text(nums, entropy, best, l) -> str:
    """DegePrime's table from the window numbers and the winning iterations (Context.dege_windows / dege_merge)."""
    lines = [HEADER]
    for pos in range(len(nums)):
        n, _, u, printed = (int(x) for x in nums[pos])
        if not printed:
            continue
        match, deg = int(best[pos, 0]), int(best[pos, 1])
        primer = "".join(SET_LETTER[int(x)] for x in best[pos, 3:3 + l])
        lines.append("\t".join((str(pos), str(n), str(u), fmt(float(entropy[pos])), str(deg), primer, str(match), fmt(match / n))))
    return "\n".join(lines) + "\n"


class DegePrime(object):
    def __init__(self, infile="", outfile="", length=18, deg=4, skip=20, depth=1, iters=100, seed=0, device=0, library=None):
        self.infile, self.outfile = infile, outfile
        self.length, self.skip, self.depth, self.iters, self.seed = int(length), int(skip), int(depth), int(iters), int(seed)
        if not DEGE_MIN_L <= self.length <= DEGE_MAX_L:
            raise DegeError(f"oligomer length {self.length}: {DEGE_MIN_L}..{DEGE_MAX_L} (one 64-bit word per oligomer)")
        if self.skip < 0 or self.depth < 1:
            raise DegeError(f"skip {self.skip} must not be negative and depth {self.depth} must be positive")
        if not 1 <= self.iters <= DEGE_MAX_ITERS:
            raise DegeError(f"{self.iters} iterations: 1..{DEGE_MAX_ITERS}")
        self.asked_deg = int(deg)
        self.deg = valid_degeneracy(self.asked_deg)
        if self.deg > 0x7FFFFFFF:
            raise DegeError(f"maximum degeneracy {self.deg}: 1..2147483647")
        self.device, self.library = device, library
        self.stats = None

    def table(self, rows) -> str:
        lib = self.library or Library()
        ctx = lib.context(self.device)
        try:
            ctx.dege_load(rows)
            nums, ent = ctx.dege_windows(self.length, self.skip, self.depth)
            best = ctx.dege_merge(self.deg, self.iters, self.seed)
            self.stats = ctx.dege_stats()
        finally:
            ctx.close()
        return table_text(nums, ent, best, self.length)

    def run(self):
        rows = read_trimmed(self.infile)
        text = self.table(rows)
        tmp = self.outfile + ".tmp"
        with open(tmp, "w") as f:
            f.write(text)
        os.rename(tmp, self.outfile)


def main(argv=None):
    p = _parser("run_dege.py", "DegePrime on the GPU (run_dege.py's flags; --skip, --depth and --iter are DegePrime.pl's)")
    p.add_argument("-i", "--input", dest="input", required=True, help="trimmed alignment (scripts/TrimAlignment.py)")
    p.add_argument("-o", "--out", dest="out", required=True, help="output table")
    p.add_argument("-s", "--script", dest="script", default=None, help="accepted and ignored (the reference's script directory)")
    p.add_argument("-l", "--length", dest="length", type=int, default=18, help="oligomer length (default 18)")
    p.add_argument("-d", "--deg", dest="deg", type=int, default=4, help="maximum degeneracy (default 4)")
    p.add_argument("--skip", "-skip", dest="skip", type=int, default=20, help="bases at both ends of a sequence that are not considered (default 20)")
    p.add_argument("--depth", "-depth", dest="depth", type=int, default=1, help="gap-free spanning sequences a window needs (default 1)")
    p.add_argument("--iter", "-iter", dest="iters", type=int, default=100, help="iterations of the merging per window (default 100)")
    p.add_argument("--seed", dest="seed", type=int, default=0, help="seed of the draws (default 0)")
    p.add_argument("--device", dest="device", type=int, default=0)
    p.add_argument("-taxfile", "--taxfile", dest="taxfile", default=None, help="not served")
    p.add_argument("-taxlevel", "--taxlevel", dest="taxlevel", default=None, help="not served")
    a = p.parse_args(argv)
    t0 = time.time()
    try:
        if a.taxfile is not None or a.taxlevel is not None:
            raise DegeError("the taxonomy columns (-taxfile / -taxlevel) are not served by this tool")
        job = DegePrime(a.input, a.out, a.length, a.deg, a.skip, a.depth, a.iters, a.seed, a.device)
        if job.deg != job.asked_deg:
            print(f"Max degeneracy was not a valid degeneracy and has been changed to {job.deg}")
        job.run()
    except DegeError as e:
        print(f"run_dege.py: {e}", file=sys.stderr)
        sys.exit(2)
    except MprimeError as e:
        if e.code != -1:                       # MP_ERR_ARG: the input is refused (a byte outside the alphabet); anything else is a fault
            raise
        print(f"run_dege.py: {e}", file=sys.stderr)
        sys.exit(2)
    ms, counts = job.stats
    print("INFO {} Total times: {} (windows {:.2f} ms, merging {:.2f} ms on the device; {} windows printed)".format(
        time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(time.time())), round(time.time() - t0, 2), ms["window_ms"], ms["merge_ms"],
        counts["printed"]))
