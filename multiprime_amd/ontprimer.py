"""Which primer pair produced each read of an amplicon sequencing run, and how many reads each pair got: the reference's
FindONTprimerV3.py / FindONTexpandprimer.py with the (reads x 2 ends) x (expanded primers x 2 strands) difflib comparisons on the GPU
(csrc/ont.hip; the rule is stated in include/mprime_ont.h and INTEGRATION.md).

    python scripts/FindONTprimer.py -i reads.fq -s primers.fa -l 18 -m 0.6 -f fq -o run
    python scripts/FindONTexpandprimer.py -i reads.fq -s primers.fa -o run

The stages are separate so that the host parts run without a GPU: key_list (the expansion over IUPAC, the reference's dict of keys, the
expand file), read_pieces (the two ends of every read, streamed in batches), rank_table / ratio_table (the reference's rounding, evaluated
by Python itself), assign (the device), Tally (names, pairs, the .num file).  Identical to the reference: the key order and labels, the
pieces (a plain file's second piece ends in its newline), the rounded ratio and the strict "> min_ident", the counts.  Different on
purpose: pairs with equal counts are written in ascending order of the pair string (the reference's order is that of a set, which
changes from run to run), and the input is streamed instead of read with readlines().
"""
from __future__ import annotations

import gzip
import os
import sys
import time
from itertools import product
from optparse import OptionParser

import numpy as np

from ._abi import ONT_MAX_LEN, ONT_Q_COLS, ONT_Q_ROWS, Library

# the bases of a degenerate letter in the order the reference expands them
DEGENERATE = {"R": "AG", "Y": "CT", "M": "AC", "K": "GT", "S": "GC", "W": "AT", "H": "ATC", "B": "GTC", "V": "GAC", "D": "GAT", "N": "ATGC"}
COMPLEMENT = str.maketrans("ACGT", "TGCA")
DEFAULT_BATCH = 1 << 18                        # reads per device call (MP_ONT_BATCH lowers it)
FORMAT_MESSAGE = "Please check your command line! -f (only fa or fq) is accepted!"


def expand(seq: str):
    """Every expansion of a degenerate sequence in itertools.product order, the leftmost degenerate position slowest."""
    return ["".join(t) for t in product(*[DEGENERATE.get(ch, ch) for ch in seq])]


def expand_name(primer_file: str) -> str:
    """The expand file's name: str.strip with the character set "fa", as the reference forms it."""
    return primer_file.strip("fa") + "expand.fa"


def key_list(primer_file: str, write: bool = True):
    """(keys, labels) in the order of the reference's dict — a key sits where it was inserted first and carries the label of its last
    insertion, so a sequence two primers produce, or one equal to its own reverse complement, appears once — and, with write, the
    expand file beside the primer file.  A primer letter that is neither A, C, G, T nor a degenerate letter is a ValueError naming
    the record: the device compares upper-case A, C, G, T only."""
    keys: dict[str, str] = {}
    text = []
    label = None
    with open(primer_file, "r") as f:
        for line in f:
            if line.startswith(">"):
                label = line.strip()
                continue
            seq = line.strip()
            if label is None:
                raise ValueError(f"{primer_file}: sequence {seq!r} before the first '>' line")
            bad = sorted(set(seq) - set("ACGT") - set(DEGENERATE))
            if bad:
                raise ValueError(f"{primer_file}: primer {label} holds {''.join(bad)!r}: upper-case A, C, G, T and the IUPAC letters "
                                 f"{''.join(DEGENERATE)} only")
            for j, s in enumerate(expand(seq)):
                if len(s) > ONT_MAX_LEN:
                    raise ValueError(f"{primer_file}: primer {label} has {len(s)} bases (at most {ONT_MAX_LEN})")
                text.append(f"{label} | {j}\n{s}\n")
                keys[s] = f"{label} | {j}"
                keys[s.translate(COMPLEMENT)[::-1]] = f"{label} | {j}"
    if write:
        with open(expand_name(primer_file), "w") as f:
            f.write("".join(text))
    return list(keys), list(keys.values())


def read_pieces(input_file: str, fmt: str, length: int, batch: int | None = None):
    """Batches of pieces, two per read in file order ([first l letters, last l letters]).  fq takes every fourth line from the second,
    fa every second one (two-line FASTA).  A .gz file's lines are decoded and stripped; a plain file's are not, so its second piece
    ends in the newline (the quirk is the reference's and is kept).  A read shorter than l gives its whole line twice."""
    if fmt not in ("fq", "fa"):
        raise ValueError(FORMAT_MESSAGE)
    if batch is None:
        batch = int(os.environ.get("MP_ONT_BATCH", "0")) or DEFAULT_BATCH
    step = 4 if fmt == "fq" else 2
    packed = input_file.endswith("gz")
    out = []
    with (gzip.open(input_file, "rb") if packed else open(input_file, "r")) as f:
        for idx, line in enumerate(f):
            if idx % step != 1:
                continue
            s = line.decode().strip() if packed else line
            out.append(s[:length])
            out.append(s[-length:])
            if len(out) >= 2 * batch:
                yield out
                out = []
    if out:
        yield out


def ratio_table() -> np.ndarray:
    """float64 [T][M]: round(2.0 * M / T, 2) as Python evaluates it (1.0 for T = 0) for the reachable M <= T / 2; a row's last
    reachable value fills the rest of it."""
    tab = np.zeros((ONT_Q_ROWS, ONT_Q_COLS), np.float64)
    for t in range(ONT_Q_ROWS):
        for m in range(ONT_Q_COLS):
            mm = min(m, t // 2)
            tab[t, m] = round(2.0 * mm / t, 2) if t else 1.0
    return tab


def rank_table(ratios: np.ndarray | None = None) -> np.ndarray:
    """int32 [T][M]: the rank of each rounded ratio among all values of the table, equal floats equal ranks — the order the device
    decides on."""
    ratios = ratio_table() if ratios is None else ratios
    values = sorted(set(ratios.reshape(-1).tolist()))
    rank = {v: i for i, v in enumerate(values)}
    return np.array([[rank[v] for v in row] for row in ratios.tolist()], np.int32)


def pack(strings):
    """(bytes uint8, offsets int64) of a list of str: one byte per character, a character outside ASCII becomes '?' (it matches no key)."""
    raw = [s.encode("ascii", "replace") for s in strings]
    off = np.zeros(len(raw) + 1, np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw), np.uint8), off


class Tally:
    """Names per piece, pairs per read, counts per pair, the .num file."""

    def __init__(self, keys, labels, min_ident: float, full_label: bool = False):
        self.key_len = np.array([len(k) for k in keys], np.int64)
        self.names = [lab if full_label else lab.split(" | ")[0] for lab in labels]
        self.min_ident = min_ident
        self.ratios = ratio_table()
        self.counts: dict[str, int] = {}

    def name(self, piece_len: int, key: int, m: int) -> str:
        return self.names[key] if self.ratios[piece_len + int(self.key_len[key]), m] > self.min_ident else "NA"

    def add(self, piece_len, key, m):
        """One batch: piece_len, key, m per piece, two consecutive pieces per read."""
        ok = self.ratios[np.asarray(piece_len, np.int64) + self.key_len[key], m] > self.min_ident
        codes = np.where(ok, key, -1).reshape(-1, 2)
        uniq, n = np.unique(codes, axis=0, return_counts=True)
        for (a, b), c in zip(uniq.tolist(), n.tolist()):
            pair = "\t".join(sorted(("NA" if a < 0 else self.names[a], "NA" if b < 0 else self.names[b])))
            self.counts[pair] = self.counts.get(pair, 0) + c

    def lines(self):
        """Count descending; among equal counts the pair string ascending."""
        return ["Primer_F\tPrimer_R\tNumber\n"] + [f"{p}\t{c}\n" for p, c in sorted(self.counts.items(), key=lambda x: (-x[1], x[0]))]

    def write(self, outfile: str):
        with open(outfile + ".num", "w") as f:
            f.write("".join(self.lines()))


class ONTprimer:
    """The reference's class: constructor arguments and run().  nproc is accepted and ignored; expand=True names a read end by the full
    label "ID | j" (FindONTexpandprimer.py)."""

    def __init__(self, input_file, primer_file, outfile="", primer_len=18, min_ident=0.8, Input_format="fq", nproc=10, expand=False,
                 library=None, device=0):
        if not 1 <= int(primer_len) <= ONT_MAX_LEN:
            raise ValueError(f"primer length {primer_len}: the device compares pieces of 1..{ONT_MAX_LEN} letters")
        self.input_file = input_file
        self.primer_file = primer_file
        self.keys, self.labels = key_list(primer_file)
        self.expand_dict = dict(zip(self.keys, self.labels))
        self.outfile = outfile
        self.Input_format = Input_format
        self.min_ident = min_ident
        self.primer_len = int(primer_len)
        self.nproc = nproc
        self.expand = expand
        self.library = library
        self.device = device
        self.stats = ({"assign_ms": 0.0}, {"keys": len(self.keys), "pieces": 0})

    def assign(self, ctx, pieces, q):
        """(piece lengths, key index, M) of one batch on the device."""
        data, off = pack(pieces)
        key, m = ctx.ont_assign(data, off, q)
        return np.diff(off), key, m

    def run(self):
        if self.Input_format not in ("fq", "fa"):
            print(FORMAT_MESSAGE)
            sys.exit(1)
        if not self.keys:
            raise ValueError(f"{self.primer_file}: no primer")
        tally = Tally(self.keys, self.labels, self.min_ident, self.expand)
        q = rank_table(tally.ratios)
        lib = self.library or Library()
        ctx = lib.context(self.device)
        try:
            ctx.ont_set_keys(*pack(self.keys))
            for pieces in read_pieces(self.input_file, self.Input_format, self.primer_len):
                tally.add(*self.assign(ctx, pieces, q))
            self.stats = ctx.ont_stats()
        finally:
            ctx.close()
        tally.write(self.outfile)
        return tally


def _parser(expand: bool):
    if expand:
        p = OptionParser("Usage: %prog -i [input] -s [primer set] -p [1] -o [output].")
    else:
        p = OptionParser("Usage: %prog -i [input] -s [primer set] -p [10] -l [primer length] -m [0.6] -f [fq] -o [output].")
    p.add_option("-i", "--input", dest="input", help="Input file: fastq or fasta, plain or .gz.")
    p.add_option("-s", "--set", dest="set", help="Primer set file.")
    p.add_option("-p", "--nproc", dest="nproc", default=1 if expand else 10, type="int",
                 help="Accepted and ignored: the comparisons run on the GPU. Default: %default")
    p.add_option("-l", "--len", dest="len", default=18, type="int", help="Primer length (1..64). Default: %default")
    p.add_option("-m", "--min_ident", dest="min_ident", default=0.8 if expand else 0.6, type="float", help="Min identity. Default: %default")
    p.add_option("-f", "--format", dest="format", default="fq", type="str", help="Input format: fa or fq (a .gz name is unpacked). Default: %default")
    p.add_option("-o", "--out", dest="out", help="Output prefix: [out].num is written.")
    return p


def main(argv=None, expand: bool = False):
    argv = sys.argv[1:] if argv is None else argv
    t0 = time.time()
    p = _parser(expand)
    options, _ = p.parse_args(argv)
    if not argv:
        p.print_help()
        sys.exit(1)
    if options.input is None:
        p.print_help()
        print("Input file must be specified !!!")
        sys.exit(1)
    if options.out is None:
        p.print_help()
        print("No output file provided !!!")
        sys.exit(1)
    if options.set is None:
        p.print_help()
        print("Primer set file must be specified !!!")
        sys.exit(1)
    try:
        app = ONTprimer(options.input, options.set, outfile=options.out, primer_len=options.len, Input_format=options.format,
                        min_ident=options.min_ident, nproc=options.nproc, expand=expand)
    except ValueError as e:
        print(f"{os.path.basename(sys.argv[0])}: {e}", file=sys.stderr)
        sys.exit(2)
    app.run()
    ms, counts = app.stats
    print("INFO {} Total times: {} ({:.2f} ms on the device; {} pieces against {} keys)".format(
        time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(time.time())), round(time.time() - t0, 2), ms["assign_ms"], counts["pieces"],
        counts["keys"]))


def expand_main(argv=None):
    main(argv, expand=True)
