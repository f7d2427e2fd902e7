"""Anchored alignment: place the unaligned sequences of a cluster on the columns of its small seed alignment, keeping the seed's
width — the step `mafft --addfragments --keeplength` does on a CPU, as one GPU pass (csrc/anchor.hip; the rule is stated in
include/mprime_anchor.h and INTEGRATION.md).  The output is an ordinary aligned FASTA for scripts/multiPrime-core.py.

    python scripts/anchor_msa.py -s cluster.tmsa -i cluster.fa -o cluster.full.tmsa

writes OUT (the seed's records, then every accepted query as one line of L letters), OUT.anchor.tsv (one line per query) and
OUT.unaligned.fa (the rejected queries as given).  Records are those of the FASTA front end every drop-in uses (msa.read_records):
an id is the header's first token, '>' included.  `--adjust-direction` (mafft's --adjustdirection): a query whose reverse complement
seeds better is turned; it is written under the id `_R_<id>`, its row is that of the reverse complement, and OUT.anchor.tsv gets a last
column `strand`.  OUT.unaligned.fa keeps queries as given.
"""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from ._abi import ANCHOR_MAX_BAND, ANCHOR_MAX_LEN, ANCHOR_MAX_PARAM, ANCHOR_REVERSED, Library

META_FIELDS = ("score", "d0", "n_match", "n_ins", "n_del", "first_col", "last_col", "status", "first_anchor", "last_anchor")
_UPPER = np.arange(256, dtype=np.uint8)
_UPPER[ord("a"):ord("z") + 1] -= 32


def anchor_of(seed_rows):
    """(anchor, col) of a seed alignment: `seed_rows` a uint8 array [R][L] (or equal-length byte strings).  Column c is an anchor column
    when strictly more than R / 2 rows hold a non-gap letter; its base is the most frequent of A, C, G, T (ties to the earlier letter),
    `N` when none occurs.  anchor: bytes of length n; col: int32 [n]."""
    if not isinstance(seed_rows, np.ndarray):
        seed_rows = np.array([np.frombuffer(bytes(r), np.uint8) for r in seed_rows], np.uint8)
    rows = _UPPER[np.ascontiguousarray(seed_rows, dtype=np.uint8)]
    n_rows = rows.shape[0]
    is_anchor = 2 * (rows != ord("-")).sum(axis=0) > n_rows
    counts = np.stack([(rows == ord(b)).sum(axis=0) for b in "ACGT"])             # [4][L]
    base = np.frombuffer(b"ACGT", np.uint8)[counts.argmax(axis=0)]                # (argmax: the first of equals)
    base = np.where(counts.max(axis=0) > 0, base, ord("N")).astype(np.uint8)
    col = np.flatnonzero(is_anchor).astype(np.int32)
    return base[col].tobytes(), col


def oriented_id(ident: str, reversed_: bool) -> str:
    """mafft's name of a record it turned: `>_R_<id>`."""
    return (">_R_" + ident[1:] if ident.startswith(">") else "_R_" + ident) if reversed_ else ident


def _records(path, what):
    from .msa import read_records
    try:
        ids, data, off = read_records(path)
    except (OSError, ValueError) as e:
        raise SystemExit(f"{what} {path}: {e}") from None
    if len(ids) == 0:
        raise SystemExit(f"{what} {path}: no records")
    return ids, data, off


class AnchoredAlignment:
    def __init__(self, seed_file, query_file, outfile, band=32, match=5, mismatch=4, gap_open=10, gap_extend=2, min_identity=0.5,
                 keep_seed=True, device=0, library=None, want_ops=False, adjust_direction=False):
        self.adjust_direction = bool(adjust_direction)
        self.seed_file, self.query_file, self.outfile = seed_file, query_file, outfile
        self.band, self.match, self.mismatch, self.gap_open, self.gap_extend = int(band), int(match), int(mismatch), int(gap_open), int(gap_extend)
        self.min_identity_permille = int(round(float(min_identity) * 1000))
        self.keep_seed, self.device, self.library, self.want_ops = keep_seed, device, library, want_ops
        if not 0 <= self.band <= ANCHOR_MAX_BAND:
            raise ValueError(f"band {self.band}: 0..{ANCHOR_MAX_BAND}")
        for name in ("match", "mismatch", "gap_open", "gap_extend"):
            if not 0 <= getattr(self, name) <= ANCHOR_MAX_PARAM:
                raise ValueError(f"{name} {getattr(self, name)}: 0..{ANCHOR_MAX_PARAM}")
        if not 0 <= self.min_identity_permille <= 1000:
            raise ValueError(f"min_identity {min_identity}: 0..1")
        self.stats = {}
        self._rows = self._meta = self._ids = self._ops = None

    # -- input ---------------------------------------------------------------------------------------------------------------------------
    def load(self):
        """Seed and queries through the FASTA front end; every refusal is raised here, before anything is launched."""
        self.seed_ids, sdata, soff = _records(self.seed_file, "seed alignment")
        widths = np.diff(soff)
        if widths.min() != widths.max() or widths[0] == 0:
            raise SystemExit(f"seed alignment {self.seed_file}: rows of {widths.min()}..{widths.max()} letters are not an alignment")
        self.width = int(widths[0])
        self.seed_rows = sdata[: soff[-1]].reshape(len(self.seed_ids), self.width)
        self.anchor, self.col = anchor_of(self.seed_rows)
        if not 1 <= len(self.anchor) <= ANCHOR_MAX_LEN:
            raise ValueError(f"seed alignment {self.seed_file}: {len(self.anchor)} anchor columns (1..{ANCHOR_MAX_LEN})")
        self._ids, self.qdata, self.qoff = _records(self.query_file, "queries")
        lens = np.diff(self.qoff)
        bad = np.flatnonzero((lens < 1) | (lens > ANCHOR_MAX_LEN))
        if len(bad):
            raise ValueError(f"query {self._ids[int(bad[0])]} has {int(lens[bad[0]])} bases (1..{ANCHOR_MAX_LEN})")

    # -- the device pass -----------------------------------------------------------------------------------------------------------------
    def align(self):
        lib = self.library or Library()
        if not lib.anchor:
            raise RuntimeError(f"{lib.path} has no anchored alignment (include/mprime_anchor.h): there is no host fallback")
        ctx = lib.context(self.device)
        try:
            if self.adjust_direction:
                ctx.anchor_strands(True)
            ctx.anchor_set(self.anchor, self.col, self.width, band=self.band, match=self.match, mismatch=self.mismatch, gap_open=self.gap_open,
                           gap_extend=self.gap_extend, min_identity_permille=self.min_identity_permille)
            self._rows, self._meta, self._ops = ctx.anchor_align(self.qdata, self.qoff, want_ops=self.want_ops)
            ms, counts = ctx.anchor_stats()
            self.stats.update(ms, **counts)
        finally:
            ctx.close()

    # -- output --------------------------------------------------------------------------------------------------------------------------
    def write(self):
        ok = (self._meta[:, 7] & 1) == 0
        with open(self.outfile, "wb") as fo:
            if self.keep_seed:
                for sid, row in zip(self.seed_ids, self.seed_rows):
                    fo.write(sid.encode() + b"\n" + row.tobytes() + b"\n")
            # header and row of every accepted query in one buffer per chunk
            for q0 in range(0, len(ok), 1 << 16):
                parts = []
                for q in np.flatnonzero(ok[q0:q0 + (1 << 16)]) + q0:
                    parts.append(oriented_id(self._ids[q], bool(self._meta[q, 7] & ANCHOR_REVERSED)).encode())
                    parts.append(self._rows[q].tobytes())
                if parts:
                    fo.write(b"\n".join(parts) + b"\n")
        with open(self.outfile + ".anchor.tsv", "w") as fo:
            strand = self.adjust_direction
            fo.write("id\tstatus\tscore\td0\tn_match\tn_ins\tn_del\tfirst_col\tlast_col" + ("\tstrand\n" if strand else "\n"))
            fo.writelines("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}{}\n".format(self._ids[q], mt[7], mt[0], mt[1], mt[2], mt[3], mt[4], mt[5], mt[6],
                                                                          ("\t-" if mt[7] & ANCHOR_REVERSED else "\t+") if strand else "")
                          for q, mt in enumerate(self._meta.tolist()))
        with open(self.outfile + ".unaligned.fa", "wb") as fo:
            for q in np.flatnonzero(~ok):
                fo.write(self._ids[q].encode() + b"\n" + self.qdata[self.qoff[q]:self.qoff[q + 1]].tobytes() + b"\n")

    def run(self):
        t0 = time.time()
        self.load()
        t1 = time.time()
        self.align()
        t2 = time.time()
        self.write()
        self.stats.update(load_s=t1 - t0, align_s=t2 - t1, write_s=time.time() - t2, n_queries=len(self._ids),
                          n_rejected=int((self._meta[:, 7] & 1).sum()), n_band_warnings=int(((self._meta[:, 7] & 2) != 0).sum()))
        return self

    # -- in-memory accessors (after run()) -----------------------------------------------------------------------------------------------
    def _ran(self):
        if self._meta is None:
            raise RuntimeError("AnchoredAlignment: run() first")

    def rows(self):
        """uint8 [n_queries][L]: the row of every query (the rejected ones included)."""
        self._ran()
        return self._rows

    def ids(self):
        self._ran()
        return list(self._ids)

    def meta(self):
        """One dict per query: score, d0, n_match, n_ins, n_del, first_col, last_col, status, first_anchor, last_anchor."""
        self._ran()
        return [dict(zip(META_FIELDS, mt)) for mt in self._meta.tolist()]

    def ops(self):
        """The op strings over M / D / I (want_ops=True), else None."""
        self._ran()
        return None if self._ops is None else [o.decode() for o in self._ops]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Place unaligned sequences on a seed alignment, keeping its width (GPU)")
    p.add_argument("-s", "--seed", required=True, metavar="<file>", help="seed alignment (aligned FASTA), or one unaligned record")
    p.add_argument("-i", "--input", required=True, metavar="<file>", help="unaligned sequences to add (FASTA)")
    p.add_argument("-o", "--out", required=True, metavar="<file>", help="aligned FASTA; <out>.anchor.tsv and <out>.unaligned.fa beside it")
    p.add_argument("--band", type=int, default=32, metavar="<int>", help=f"half width W of the band around the seed diagonal, 0..{ANCHOR_MAX_BAND}. Default: 32")
    p.add_argument("--match", type=int, default=5, metavar="<int>")
    p.add_argument("--mismatch", type=int, default=4, metavar="<int>")
    p.add_argument("--gap-open", type=int, default=10, metavar="<int>")
    p.add_argument("--gap-extend", type=int, default=2, metavar="<int>")
    p.add_argument("--min-identity", type=float, default=0.5, metavar="<float>",
                   help="a query with fewer matching pairs than this share of its length goes to <out>.unaligned.fa. Default: 0.5")
    p.add_argument("--no-seed", action="store_true", help="do not repeat the seed's records in <out>")
    p.add_argument("--adjust-direction", action="store_true", help="turn a query whose reverse complement seeds better (mafft --adjustdirection); "
                   "it is written as _R_<id>. Default: queries are aligned as given")
    p.add_argument("--device", type=int, default=0, help="GPU ordinal (default 0)")
    args = p.parse_args(argv)
    if not 0 <= args.band <= ANCHOR_MAX_BAND:
        p.error(f"--band must be in 0..{ANCHOR_MAX_BAND}")
    for name in ("match", "mismatch", "gap_open", "gap_extend"):
        if not 0 <= getattr(args, name) <= ANCHOR_MAX_PARAM:
            p.error(f"--{name.replace('_', '-')} must be in 0..{ANCHOR_MAX_PARAM}")
    if not 0 <= args.min_identity <= 1:
        p.error("--min-identity must be in 0..1")
    return args


def main(argv=None):
    from ._abi import prefer_staged_copies
    prefer_staged_copies()                      # a command line owns its process: see _abi.prefer_staged_copies
    e1 = time.time()
    args = parse_args(argv)                     # exit status 2 on bad flags
    app = AnchoredAlignment(args.seed, args.input, args.out, band=args.band, match=args.match, mismatch=args.mismatch, gap_open=args.gap_open,
                            gap_extend=args.gap_extend, min_identity=args.min_identity, keep_seed=not args.no_seed, device=args.device,
                            adjust_direction=args.adjust_direction)
    try:
        app.run()                               # SystemExit with a message (status 1) on an unreadable or empty input
    except ValueError as e:
        print(e, file=sys.stderr)
        sys.exit(1)
    e2 = time.time()
    print("INFO {} Total times: {}".format(time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(time.time())), round(float(e2 - e1), 2)))
