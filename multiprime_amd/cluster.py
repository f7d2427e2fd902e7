"""Clustering by identity: greedy incremental clustering of unaligned sequences on the GPU — the two `cd-hit` calls of the pipeline
(`-c 1`, duplicate removal, and `-c <identity>`, rule cluster_by_identity) as one tool (csrc/cluster.hip; the rule is stated in
include/mprime_cluster.h and INTEGRATION.md).

    python scripts/cluster_by_identity.py -i in.fa -o out.fa -c 0.8

(`--both-strands`: a record may also join as its reverse complement, cd-hit-est's `-r 1`; member lines then read `at +/dd.dd%` or
`at -/dd.dd%`) writes OUT (the representatives' records in cluster order, upper-cased, one line each) and OUT.clstr in cd-hit's layout, which is what
extract_cluster.py parses.  Records are those of the FASTA front end every drop-in uses (msa.read_records): an id is the header's first
token, '>' included.
"""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from ._abi import ANCHOR_MAX_BAND, ANCHOR_MAX_LEN, ANCHOR_MAX_PARAM, Library

_UPPER = np.arange(256, dtype=np.uint8)
_UPPER[ord("a"):ord("z") + 1] -= 32


def identity_text(n_match: int, m: int) -> str:
    """(n_match * 10000 + m / 2) / m in integers, as dd.dd%."""
    v = (int(n_match) * 10000 + int(m) // 2) // int(m)
    return "%d.%02d%%" % (v // 100, v % 100)


class ClusterByIdentity:
    def __init__(self, input, outfile, identity=0.8, band=32, min_votes=1, match=5, mismatch=4, gap_open=10, gap_extend=2, device=0,
                 library=None, both_strands=False):
        self.input, self.outfile = input, outfile
        self.identity_permille = int(round(float(identity) * 1000))
        self.band, self.min_votes = int(band), int(min_votes)
        self.match, self.mismatch, self.gap_open, self.gap_extend = int(match), int(mismatch), int(gap_open), int(gap_extend)
        self.device, self.library, self.both_strands = device, library, bool(both_strands)
        if not 0 <= self.identity_permille <= 1000:
            raise ValueError(f"identity {identity}: 0..1")
        if not 0 <= self.band <= ANCHOR_MAX_BAND:
            raise ValueError(f"band {self.band}: 0..{ANCHOR_MAX_BAND}")
        if not 0 <= self.min_votes <= ANCHOR_MAX_LEN:
            raise ValueError(f"min_votes {self.min_votes}: 0..{ANCHOR_MAX_LEN}")
        for name in ("match", "mismatch", "gap_open", "gap_extend"):
            if not 0 <= getattr(self, name) <= ANCHOR_MAX_PARAM:
                raise ValueError(f"{name} {getattr(self, name)}: 0..{ANCHOR_MAX_PARAM}")
        self.stats = {}
        self._ids = self._cluster_of = self._reps = self._n_match = self._strand = None

    def _params(self):
        return dict(band=self.band, identity_permille=self.identity_permille, min_votes=self.min_votes, match=self.match, mismatch=self.mismatch,
                    gap_open=self.gap_open, gap_extend=self.gap_extend)

    # -- input ---------------------------------------------------------------------------------------------------------------------------
    def load(self):
        """The records through the FASTA front end; every refusal is raised here, before anything is launched."""
        from .msa import read_records
        try:
            self._ids, self.data, self.off = read_records(self.input)
        except (OSError, ValueError) as e:
            raise SystemExit(f"input {self.input}: {e}") from None
        if len(self._ids) == 0:
            raise SystemExit(f"input {self.input}: no records")
        self.lens = np.diff(self.off)
        bad = np.flatnonzero((self.lens < 1) | (self.lens > ANCHOR_MAX_LEN))
        if len(bad):
            raise ValueError(f"record {self._ids[int(bad[0])]} has {int(self.lens[bad[0]])} bases (1..{ANCHOR_MAX_LEN})")

    # -- the device pass -----------------------------------------------------------------------------------------------------------------
    def cluster(self):
        lib = self.library or Library()
        if not lib.cluster:
            raise RuntimeError(f"{lib.path} has no clustering (include/mprime_cluster.h): there is no host fallback")
        ctx = lib.context(self.device)
        try:
            ctx.cluster_load(self.data, self.off)
            if self.both_strands:
                self._cluster_of, self._reps, self._n_match, self._strand = ctx.cluster_greedy_strands(**self._params())
            else:
                self._cluster_of, self._reps, self._n_match = ctx.cluster_greedy(**self._params())
            ms, counts = ctx.cluster_stats()
            self.stats.update(ms, **counts)
        finally:
            ctx.close()

    # -- output --------------------------------------------------------------------------------------------------------------------------
    def clstr_text(self) -> str:
        """The .clstr file: `>Cluster k`, then the members in input order, numbered from 0."""
        order = np.argsort(self._cluster_of, kind="stable")
        is_rep = np.zeros(len(self._ids), bool)
        is_rep[self._reps] = True
        lines, last, x = [], -1, 0
        for i in order.tolist():
            k = int(self._cluster_of[i])
            if k != last:
                lines.append(">Cluster %d" % k)
                last, x = k, 0
            sign = ("-/" if self._strand[i] else "+/") if self.both_strands else ""
            tail = "*" if is_rep[i] else "at " + sign + identity_text(self._n_match[i], self.lens[i])
            lines.append("%d\t%daa, %s... %s" % (x, self.lens[i], self._ids[i], tail))
            x += 1
        return "\n".join(lines) + "\n"

    def write(self):
        with open(self.outfile, "wb") as fo:
            for i in self._reps.tolist():
                fo.write(self._ids[i].encode() + b"\n" + _UPPER[self.data[self.off[i]:self.off[i + 1]]].tobytes() + b"\n")
        with open(self.outfile + ".clstr", "w") as fo:
            fo.write(self.clstr_text())

    def run(self):
        t0 = time.time()
        self.load()
        t1 = time.time()
        self.cluster()
        t2 = time.time()
        self.write()
        self.stats.update(load_s=t1 - t0, cluster_s=t2 - t1, write_s=time.time() - t2, n_records=len(self._ids), n_clusters=len(self._reps))
        return self

    # -- in-memory accessors (after run()) -----------------------------------------------------------------------------------------------
    def _ran(self):
        if self._cluster_of is None:
            raise RuntimeError("ClusterByIdentity: run() first")

    def ids(self):
        self._ran()
        return list(self._ids)

    def cluster_of(self):
        """int32 [n]: the cluster number of every record."""
        self._ran()
        return self._cluster_of

    def representatives(self):
        """int32 [n_clusters]: the record that founded each cluster."""
        self._ran()
        return self._reps

    def n_match(self):
        """int32 [n]: a member's matching pairs against its representative (a representative: its length)."""
        self._ran()
        return self._n_match

    @property
    def strand(self):
        """int32 [n]: 1 where a member joined as its reverse complement (representatives and forward members 0); None without both_strands."""
        self._ran()
        return self._strand


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Cluster sequences by identity (greedy incremental, cd-hit's .clstr layout) on the GPU")
    p.add_argument("-i", "--input", required=True, metavar="<file>", help="sequences (FASTA)")
    p.add_argument("-o", "--out", required=True, metavar="<file>", help="representatives (FASTA); <out>.clstr beside it")
    p.add_argument("-c", "--identity", type=float, default=0.8, metavar="<float>", help="identity threshold over the shorter sequence. Default: 0.8")
    p.add_argument("--band", type=int, default=32, metavar="<int>", help=f"half width W of the band around the seed diagonal, 0..{ANCHOR_MAX_BAND}. Default: 32")
    p.add_argument("--min-votes", type=int, default=1, metavar="<int>", help="shared 12-mers on the best diagonal a pair needs to be aligned. Default: 1")
    p.add_argument("--both-strands", action="store_true", help="a record may join a cluster as its reverse complement (cd-hit-est -r 1); "
                   "member lines read `at +/dd.dd%%` / `at -/dd.dd%%`. Default: forward strand only")
    p.add_argument("--match", type=int, default=5, metavar="<int>")
    p.add_argument("--mismatch", type=int, default=4, metavar="<int>")
    p.add_argument("--gap-open", type=int, default=10, metavar="<int>")
    p.add_argument("--gap-extend", type=int, default=2, metavar="<int>")
    p.add_argument("--device", type=int, default=0, help="GPU ordinal (default 0)")
    args = p.parse_args(argv)
    if not 0 <= args.identity <= 1:
        p.error("-c must be in 0..1")
    if not 0 <= args.band <= ANCHOR_MAX_BAND:
        p.error(f"--band must be in 0..{ANCHOR_MAX_BAND}")
    if not 0 <= args.min_votes <= ANCHOR_MAX_LEN:
        p.error(f"--min-votes must be in 0..{ANCHOR_MAX_LEN}")
    for name in ("match", "mismatch", "gap_open", "gap_extend"):
        if not 0 <= getattr(args, name) <= ANCHOR_MAX_PARAM:
            p.error(f"--{name.replace('_', '-')} must be in 0..{ANCHOR_MAX_PARAM}")
    return args


def main(argv=None):
    from ._abi import prefer_staged_copies
    prefer_staged_copies()                      # a command line owns its process: see _abi.prefer_staged_copies
    e1 = time.time()
    args = parse_args(argv)                     # exit status 2 on bad flags
    app = ClusterByIdentity(args.input, args.out, identity=args.identity, band=args.band, min_votes=args.min_votes, match=args.match,
                            mismatch=args.mismatch, gap_open=args.gap_open, gap_extend=args.gap_extend, device=args.device,
                            both_strands=args.both_strands)
    try:
        app.run()                               # SystemExit with a message (status 1) on an unreadable or empty input
    except ValueError as e:
        print(e, file=sys.stderr)
        sys.exit(1)
    e2 = time.time()
    print("INFO {} Total times: {}".format(time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(time.time())), round(float(e2 - e1), 2)))
