"""Star alignment: build a cluster's alignment from nothing on the GPU — the step `mafft --auto` does in the reference workflow
(scripts/run_mafft.py -i X.tfa -o X.tmsa), with every inserted base kept (csrc/star.hip; the rule is stated in include/mprime_star.h
and INTEGRATION.md).  The output is an ordinary aligned FASTA for scripts/multiPrime-core.py.

    python scripts/run_mafft.py -i cluster.tfa -o cluster.tmsa

writes OUT (the placed records in input order, one line of L' letters each), OUT.star.tsv (one line per record, then one `#` line
per round) and OUT.unaligned.fa (the unplaced records as given).  Records are those of the FASTA front end every drop-in uses
(msa.read_records): an id is the header's first token, '>' included.  The round loop lives here: round 0's anchor is the longest
record, every later one the majority consensus of the round before, computed from the column counts the device hands back.
`--adjust-direction` (mafft's --adjustdirection): every round votes both strands of a record and turns it where its reverse complement
seeds better; a turned record is written under the id `_R_<id>`, its row is that of the reverse complement, and OUT.star.tsv gets a last
column `strand`.  OUT.unaligned.fa keeps records as given.
"""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from ._abi import ANCHOR_MAX_BAND, ANCHOR_MAX_LEN, ANCHOR_MAX_PARAM, ANCHOR_REVERSED, STAR_MAX_ROUNDS, Library

META_FIELDS = ("score", "d0", "n_match", "n_ins", "n_del", "first_col", "last_col", "status", "first_anchor", "last_anchor", "band")
_UPPER = np.arange(256, dtype=np.uint8)
_UPPER[ord("a"):ord("z") + 1] -= 32


def oriented_id(ident: str, reversed_: bool) -> str:
    """mafft's name of a record it turned: `>_R_<id>`."""
    return (">_R_" + ident[1:] if ident.startswith(">") else "_R_" + ident) if reversed_ else ident


def anchor_of_counts(counts, placed):
    """The next anchor from the column counts [L'][6] (A, C, G, T, other letter, gap) of `placed` rows: the rule of anchor.anchor_of."""
    counts = np.asarray(counts, np.int64)
    letters = counts[:, :5].sum(axis=1)
    is_anchor = 2 * letters > placed
    base = np.frombuffer(b"ACGT", np.uint8)[counts[:, :4].argmax(axis=1)]          # (argmax: the first of equals)
    base = np.where(counts[:, :4].max(axis=1) > 0, base, ord("N")).astype(np.uint8)
    return base[is_anchor].tobytes()


class StarAlignment:
    def __init__(self, infile, outfile, rounds=2, band=32, match=5, mismatch=4, gap_open=10, gap_extend=2, min_identity=0.5, device=0,
                 library=None, adjust_direction=False):
        self.infile, self.outfile = infile, outfile
        self.adjust_direction = bool(adjust_direction)
        self.rounds, self.band = int(rounds), int(band)
        self.match, self.mismatch, self.gap_open, self.gap_extend = int(match), int(mismatch), int(gap_open), int(gap_extend)
        self.min_identity_permille = int(round(float(min_identity) * 1000))
        self.device, self.library = device, library
        if not 1 <= self.rounds <= STAR_MAX_ROUNDS:
            raise ValueError(f"rounds {self.rounds}: 1..{STAR_MAX_ROUNDS}")
        if not 1 <= self.band <= ANCHOR_MAX_BAND:
            raise ValueError(f"band {self.band}: 1..{ANCHOR_MAX_BAND}")
        for name in ("match", "mismatch", "gap_open", "gap_extend"):
            if not 0 <= getattr(self, name) <= ANCHOR_MAX_PARAM:
                raise ValueError(f"{name} {getattr(self, name)}: 0..{ANCHOR_MAX_PARAM}")
        if not 0 <= self.min_identity_permille <= 1000:
            raise ValueError(f"min_identity {min_identity}: 0..1")
        self.stats = {}
        self.round_stats = []
        self._rows = self._meta = self._ids = self._anchors = None

    # -- input ---------------------------------------------------------------------------------------------------------------------------
    def load(self):
        """The records through the FASTA front end, `-` and `.` removed; every refusal is raised here, before anything is launched."""
        from .anchor import _records
        self._ids, data, off = _records(self.infile, "input")
        self.raw, self.raw_off = data, off
        keep = (data[: off[-1]] != ord("-")) & (data[: off[-1]] != ord("."))
        kept = np.zeros(len(keep) + 1, np.int64)
        np.cumsum(keep, out=kept[1:])
        self.data, self.off = np.ascontiguousarray(data[: off[-1]][keep]), kept[off]
        lens = np.diff(self.off)
        bad = np.flatnonzero((lens < 1) | (lens > ANCHOR_MAX_LEN))
        if len(bad):
            raise ValueError(f"record {self._ids[int(bad[0])]} has {int(lens[bad[0]])} bases (1..{ANCHOR_MAX_LEN})")
        self.centre = int(np.argmax(lens))              # the longest record, the earliest among equals

    # -- the device rounds ---------------------------------------------------------------------------------------------------------------
    def align(self):
        lib = self.library or Library()
        if not lib.star:
            raise RuntimeError(f"{lib.path} has no star alignment (include/mprime_star.h): there is no host fallback")
        ctx = lib.context(self.device)
        try:
            if self.adjust_direction:
                ctx.anchor_strands(True)
            ctx.star_load(self.data, self.off)
            anchor = _UPPER[self.data[self.off[self.centre]:self.off[self.centre + 1]]].tobytes()
            self._anchors, self.round_stats = [], []
            for k in range(self.rounds):
                meta, ins, width = ctx.star_round(anchor, band=self.band, match=self.match, mismatch=self.mismatch, gap_open=self.gap_open,
                                                  gap_extend=self.gap_extend, min_identity_permille=self.min_identity_permille)
                ms, counts = ctx.star_stats()
                self._anchors.append(anchor)
                self._meta, self._ins, self.width = meta, ins, width
                self.round_stats.append(dict(ms, **counts, n=len(anchor), width=width, band_warnings=int(((meta[:, 7] & 2) != 0).sum())))
                if k + 1 == self.rounds:
                    break
                placed = counts["placed"]
                if placed == 0:
                    raise ValueError(f"round {k}: no record placed")
                self._counts = ctx.star_counts()
                nxt = anchor_of_counts(self._counts, placed)
                if not 1 <= len(nxt) <= ANCHOR_MAX_LEN:
                    raise ValueError(f"round {k}: a consensus of {len(nxt)} letters (1..{ANCHOR_MAX_LEN})")
                if nxt == anchor:
                    break
                anchor = nxt
            self._rows = ctx.star_rows()
        finally:
            ctx.close()

    # -- output --------------------------------------------------------------------------------------------------------------------------
    def write(self):
        ok = (self._meta[:, 7] & 1) == 0
        with open(self.outfile, "wb") as fo:
            for q0 in range(0, len(ok), 1 << 16):
                parts = []
                for q in np.flatnonzero(ok[q0:q0 + (1 << 16)]) + q0:
                    parts.append(oriented_id(self._ids[q], bool(self._meta[q, 7] & ANCHOR_REVERSED)).encode())
                    parts.append(self._rows[q].tobytes())
                if parts:
                    fo.write(b"\n".join(parts) + b"\n")
        with open(self.outfile + ".star.tsv", "w") as fo:
            strand = self.adjust_direction
            fo.write("id\tstatus\tband\tscore\td0\tn_match\tn_ins\tn_del" + ("\tstrand\n" if strand else "\n"))
            fo.writelines("{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}{}\n".format(self._ids[q], mt[7], mt[10], mt[0], mt[1], mt[2], mt[3], mt[4],
                                                                      ("\t-" if mt[7] & ANCHOR_REVERSED else "\t+") if strand else "")
                          for q, mt in enumerate(self._meta.tolist()))
            for k, st in enumerate(self.round_stats):
                fo.write("# round {}: n {} width {} placed {} band_warnings {}\n".format(k, st["n"], st["width"], st["placed"], st["band_warnings"]))
        with open(self.outfile + ".unaligned.fa", "wb") as fo:
            for q in np.flatnonzero(~ok):
                fo.write(self._ids[q].encode() + b"\n" + self.raw[self.raw_off[q]:self.raw_off[q + 1]].tobytes() + b"\n")

    def run(self):
        t0 = time.time()
        self.load()
        t1 = time.time()
        self.align()
        t2 = time.time()
        self.write()
        self.stats.update(load_s=t1 - t0, align_s=t2 - t1, write_s=time.time() - t2, n_records=len(self._ids), rounds=len(self._anchors),
                          n_unplaced=int((self._meta[:, 7] & 1).sum()), n_band_warnings=int(((self._meta[:, 7] & 2) != 0).sum()))
        return self

    # -- in-memory accessors (after align() / run()) -------------------------------------------------------------------------------------
    def _ran(self):
        if self._meta is None:
            raise RuntimeError("StarAlignment: run() first")

    def rows(self):
        """uint8 [n_records][L']: the row of every record of the last round (all-gap for the unplaced ones)."""
        self._ran()
        return self._rows

    def ids(self):
        self._ran()
        return list(self._ids)

    def meta(self):
        """One dict per record of the last round: the fields of AnchoredAlignment.meta() (columns are anchor positions) and `band`."""
        self._ran()
        return [dict(zip(META_FIELDS, mt)) for mt in self._meta.tolist()]

    def anchors(self):
        """The anchor of every round that ran, as bytes."""
        self._ran()
        return list(self._anchors)

    def ins(self):
        """int32 [n + 1]: the widest inserted run per slot of the last round."""
        self._ran()
        return self._ins


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Align the records of a cluster from nothing, keeping every base (star alignment on the GPU)")
    p.add_argument("-i", "--input", required=True, metavar="<file>", help="unaligned sequences (FASTA)")
    p.add_argument("-o", "--out", required=True, metavar="<file>", help="aligned FASTA; <out>.star.tsv and <out>.unaligned.fa beside it")
    p.add_argument("--rounds", type=int, default=2, metavar="<int>", help=f"rounds, 1..{STAR_MAX_ROUNDS}: the first against the longest record, "
                   "every later one against the consensus of the round before. Default: 2")
    p.add_argument("--band", type=int, default=32, metavar="<int>", help=f"half width W of the band around the seed diagonal, 1..{ANCHOR_MAX_BAND}; "
                   "doubled for a record whose path touches it. Default: 32")
    p.add_argument("--match", type=int, default=5, metavar="<int>")
    p.add_argument("--mismatch", type=int, default=4, metavar="<int>")
    p.add_argument("--gap-open", type=int, default=10, metavar="<int>")
    p.add_argument("--gap-extend", type=int, default=2, metavar="<int>")
    p.add_argument("--min-identity", type=float, default=0.5, metavar="<float>",
                   help="a record with fewer matching pairs than this share of its length goes to <out>.unaligned.fa. Default: 0.5")
    p.add_argument("--adjust-direction", action="store_true", help="turn a record whose reverse complement seeds better (mafft --adjustdirection); "
                   "it is written as _R_<id>. Default: records are aligned as given")
    p.add_argument("--device", type=int, default=0, help="GPU ordinal (default 0)")
    args = p.parse_args(argv)
    if not 1 <= args.rounds <= STAR_MAX_ROUNDS:
        p.error(f"--rounds must be in 1..{STAR_MAX_ROUNDS}")
    if not 1 <= args.band <= ANCHOR_MAX_BAND:
        p.error(f"--band must be in 1..{ANCHOR_MAX_BAND}")
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
    app = StarAlignment(args.input, args.out, rounds=args.rounds, band=args.band, match=args.match, mismatch=args.mismatch,
                        gap_open=args.gap_open, gap_extend=args.gap_extend, min_identity=args.min_identity, device=args.device,
                        adjust_direction=args.adjust_direction)
    try:
        app.run()                               # SystemExit with a message (status 1) on an unreadable or empty input
    except ValueError as e:
        print(e, file=sys.stderr)
        sys.exit(1)
    e2 = time.time()
    print("INFO {} Total times: {}".format(time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(time.time())), round(float(e2 - e1), 2)))
