"""Merging rare clusters by average nucleotide identity on the GPU — the pipeline's merge_cluster_by_ANI.py, which runs
`fastANI --ql A.txt --rl B.txt` for every (rare cluster, larger cluster) combination, as one tool without the binary
(csrc/ani.hip; the rule is stated in include/mprime_ani.h and INTEGRATION.md).

    python scripts/merge_cluster_by_ANI.py -i results/cluster.txt -p 20 -t 20 -o results/history.txt -d F -a 0.8

runs after extract_cluster.py and works on the tree it left: `cluster.txt` and, beside it, `Clusters_fa/` with name_size.fa / .tfa /
.txt per cluster and one directory of per-sequence files per cluster.  A cluster's sequences are the records of its .tfa: with the
workflow's `extract_cluster.py -m 500` that is the set of files the .txt lists for fastANI; with `-m 0` the .tfa holds the whole cluster
while the .txt lists at most 500 of its records, so there every record counts.

The decision mirrors the reference (merge_cluster_app / high_ANI_selection) with one documented difference: the reference compares
fastANI's identity in PERCENT with `-a 0.8`, so any pair fastANI reports merges; here -a is a fraction compared with the mean as a
fraction, and --report-floor (default 0.7) is what "reported" means.  With -a <= floor the decisions are the reference's.

--both-strands compares canonical sketches (fastANI maps both strands: a rare cluster that is the reverse complement of a larger one's
neighbour merges), votes the strand of every decided merge from the sketches' orientation bits and writes <out>.strand; --orient
appends a cluster merged on the other strand reverse-complemented.  Off by default, and then nothing changes.
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys
import time

import numpy as np

from . import iupac
from ._abi import ANCHOR_MAX_LEN, ANI_MAX_SKETCH, ANI_MIN_SKETCH, ANI_PPM, Library

_EXTS = (".fa", ".tfa", ".txt")
# the complement of iupac.py, for bytes, lower case to lower case; any other byte stays
_COMP = bytes.maketrans(*(("".join(chr(k) for k in iupac._COMP) + "".join(chr(k).lower() for k in iupac._COMP)).encode(),
                          ("".join(chr(v) for v in iupac._COMP.values()) + "".join(chr(v).lower() for v in iupac._COMP.values())).encode()))


def revcomp_fasta(src, dst):
    """Append the FASTA file src to dst with every record reverse-complemented: a header line ('>') byte for byte, the record's
    sequence lines joined (stripped of white space at their ends), reversed and complemented, on one line."""
    with open(src, "rb") as fi, open(dst, "ab") as fo:
        seq = None                              # the sequence lines of the record being read; None before the first line of one

        def flush():
            if seq is not None:
                fo.write(b"".join(seq).translate(_COMP)[::-1] + b"\n")
        for line in fi:
            if line.startswith(b">"):
                flush()
                seq = None
                fo.write(line if line.endswith(b"\n") else line + b"\n")
            elif line.strip():
                seq = (seq or []) + [line.strip()]
        flush()


def _read_tfa(path):
    """[(id, sequence bytes)]: a '>' line names a record by its first token, every other line is stripped and appended."""
    out = []
    with open(path, "rb") as f:
        for line in f:
            line = line.strip()
            if line.startswith(b">"):
                out.append([line.split()[0].decode("latin-1") if len(line) > 1 else ">", []])
            elif line and out:
                out[-1][1].append(line)
    return [(i, b"".join(s)) for i, s in out]


class merge_clstr(object):
    def __init__(self, inputfile="", output="", threshold=20, drop="T", ani=0.8, nproc=10, sketch_size=ANI_MAX_SKETCH, report_floor=0.7,
                 device=0, library=None, clusters=None, both_strands=False, orient=False):
        """`clusters`: [(name, size)] instead of reading `inputfile` — with load_records(), the device pass and decide() for a caller
        that holds the records in memory (apply() still works on the files)."""
        self.cluster_file = inputfile
        self.threshold = int(threshold)
        self.work_dir = self.parse_work_dir()
        self.out = output
        self.drop = drop
        self.nproc = nproc                      # accepted and ignored: the comparison runs on the device
        self.ani = float(ani)
        self.sketch_size, self.report_floor = int(sketch_size), float(report_floor)
        self.device, self.library = device, library
        self.both_strands, self.orient = bool(both_strands), bool(orient)
        if self.orient and (not self.both_strands or drop == "T"):
            raise ValueError("orient needs both_strands and a merge (-d other than T)")
        self.strands = None                     # {(ref id, sub id): ('+' | '-', SAME, OPP)} of the decided merges (both_strands)
        if not ANI_MIN_SKETCH <= self.sketch_size <= ANI_MAX_SKETCH:
            raise ValueError(f"sketch size {self.sketch_size}: {ANI_MIN_SKETCH}..{ANI_MAX_SKETCH}")
        if not 0 <= self.ani <= 1:
            raise ValueError(f"-a {ani}: 0..1")
        if not 0 <= self.report_floor <= 1:
            raise ValueError(f"report floor {report_floor}: 0..1")
        self.ani_ppm = int(round(self.ani * ANI_PPM))
        self.report_ppm = int(round(self.report_floor * ANI_PPM))
        self.cluster = self.parse_cluster() if clusters is None else sorted(((str(k), int(n)) for k, n in clusters), key=lambda x: x[1], reverse=True)
        self.stats = {}
        self.merge_dict = None
        self._off = None

    def parse_work_dir(self):
        return self.cluster_file.rstrip("cluster.txt") + "Clusters_fa"      # (a character-set strip: the reference's, kept)

    def parse_cluster(self):
        """[(name, size)] by size descending, ties in file order."""
        d = {}
        try:
            with open(self.cluster_file, "r") as f:
                for line in f:
                    if not line.startswith("#"):
                        x = line.strip().split("\t")
                        d[x[0]] = int(x[1])
        except (OSError, ValueError, IndexError) as e:
            raise SystemExit(f"input {self.cluster_file}: {e}") from None
        return sorted(d.items(), key=lambda x: x[1], reverse=True)

    def ident(self, x):
        return self.work_dir + "/" + self.cluster[x][0] + "_" + str(self.cluster[x][1])

    def visiting(self):
        """Positions of the processing clusters, from the end of the sorted list."""
        if self.threshold == 1:
            return []
        return [p for p in range(len(self.cluster) - 1, -1, -1) if self.threshold == 0 or self.cluster[p][1] <= self.threshold]

    # -- input ---------------------------------------------------------------------------------------------------------------------------
    def load(self):
        """Every cluster's .tfa; every refusal is raised here, before anything is launched or any file is touched."""
        chunks, lens, group_off = [], [], [0]
        for x in range(len(self.cluster)):
            path = self.ident(x) + ".tfa"
            try:
                records = _read_tfa(path)
            except OSError as e:
                raise SystemExit(f"cluster file {path}: {e}") from None
            if not records:
                raise SystemExit(f"cluster file {path}: no records")
            for rid, seq in records:
                if len(seq) > ANCHOR_MAX_LEN:
                    raise SystemExit(f"cluster file {path}: record {rid} has {len(seq)} bases (at most {ANCHOR_MAX_LEN})")
                chunks.append(seq)
                lens.append(len(seq))
            group_off.append(len(lens))
        off = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        self.load_records(np.frombuffer(b"".join(chunks), np.uint8) if lens else np.zeros(0, np.uint8), off, group_off)

    def load_records(self, data, off, group_off):
        """What load() reads from the files, from memory: record i is data[off[i]:off[i+1]], and cluster x of self.cluster (the
        size-sorted list) holds the records group_off[x] .. group_off[x+1]."""
        off, group_off = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(group_off, dtype=np.int32)
        if len(group_off) != len(self.cluster) + 1 or group_off[0] != 0 or group_off[-1] != len(off) - 1 or (np.diff(group_off) < 0).any():
            raise ValueError("load_records: group_off does not split the records into the clusters of the list")
        bad = np.flatnonzero(np.diff(off) > ANCHOR_MAX_LEN)
        if len(bad):
            raise ValueError(f"load_records: record {int(bad[0])} has {int(np.diff(off)[bad[0]])} bases (at most {ANCHOR_MAX_LEN})")
        self._data, self._off, self._group_off = np.ascontiguousarray(data, dtype=np.uint8), off, group_off

    # -- the device pass -----------------------------------------------------------------------------------------------------------------
    def compare(self):
        """{(p, r): (n_rep, sum_ppm)} for every cluster pair the decision looks at: blocks of refs in list order against the processing
        clusters still undecided; a processing cluster leaves once a ref of a block takes it.  The block size (MP_ANI_REF_BLOCK caps
        it) changes which pairs are evaluated beyond the deciding one, never the decision."""
        if self._off is None:
            raise RuntimeError("merge_clstr: load() first")
        numbers = {}
        if self.both_strands:
            self.strands = {}
            self.stats.update(strand_ms=0.0, n_minus=0)
        todo = self.visiting()
        if not todo or len(self._off) < 2:
            return numbers
        lib = self.library or Library()
        if not lib.ani:
            raise RuntimeError(f"{lib.path} has no identity merge (include/mprime_ani.h): there is no host fallback")
        block = 256
        if os.environ.get("MP_ANI_REF_BLOCK"):
            block = max(1, min(block, int(os.environ["MP_ANI_REF_BLOCK"])))
        size = [n for _, n in self.cluster]
        ctx = lib.context(self.device)
        try:
            if self.both_strands:
                ctx.ani_sketch(self._data, self._off, self.sketch_size, strands=True)
            else:
                ctx.ani_sketch(self._data, self._off, self.sketch_size)
            for r0 in range(0, len(self.cluster), block):
                if not todo:
                    break
                refs = range(r0, min(r0 + block, len(self.cluster)))
                q = [p for p in todo for r in refs if size[r] > size[p]]
                r = [r for p in todo for r in refs if size[r] > size[p]]
                if not q:
                    continue
                got = ctx.ani_groups(self._group_off, q, r, self.report_ppm).tolist()
                taken = set()
                for p, rr, (n_rep, total) in zip(q, r, got):
                    numbers[(p, rr)] = (n_rep, total)
                    if n_rep > 0 and total >= self.ani_ppm * n_rep:
                        taken.add(p)
                todo = [p for p in todo if p not in taken]
            ms, counts = ctx.ani_stats()
            self.stats.update(ms, **counts)
            if self.both_strands:
                self.vote(ctx, numbers)
        finally:
            ctx.close()
        return numbers

    def vote(self, ctx, numbers):
        """The strand of every merge decide() takes from `numbers`: one ani_groups_strand call over the decided (sub, ref) pairs on
        the resident canonical set fills self.strands."""
        kept = self.merge_dict
        pos = {self.ident(x): x for x in range(len(self.cluster))}
        pairs = [(ref, sub) for ref, subs in self.decide(numbers).items() for sub in subs]
        self.merge_dict = kept
        self.strands = {}
        t0 = time.time()
        if pairs:
            got = ctx.ani_groups_strand(self._group_off, [pos[sub] for _, sub in pairs], [pos[ref] for ref, _ in pairs], self.report_ppm).tolist()
            for key, (same, opp) in zip(pairs, got):
                self.strands[key] = ("-" if opp > same else "+", same, opp)
        self.stats.update(strand_ms=(time.time() - t0) * 1e3, n_minus=sum(v[0] == "-" for v in self.strands.values()))

    # -- the decision --------------------------------------------------------------------------------------------------------------------
    def decide(self, numbers):
        """numbers: {(p, r): (n_rep, sum_ppm)} or a callable (p, r) -> (n_rep, sum_ppm), p and r positions in self.cluster.  A
        processing cluster merges into the first larger cluster, from the front of the list, with n_rep > 0 and a mean of at least -a;
        pairs behind that one are not looked up.  Sets and returns merge_dict {ref id: [sub id]}: refs in order of first appearance,
        subs in visiting order."""
        get = numbers if callable(numbers) else (lambda p, r: numbers[(p, r)])
        md = {}
        for p in self.visiting():
            for r in range(len(self.cluster)):
                if self.cluster[r][1] > self.cluster[p][1]:
                    n_rep, total = get(p, r)
                    if n_rep > 0 and total >= self.ani_ppm * n_rep:
                        md.setdefault(self.ident(r), []).append(self.ident(p))
                        break
        self.merge_dict = md
        return md

    def write_history(self):
        with open(self.out, "w") as f:
            for k, subs in self.merge_dict.items():
                for m in subs:
                    f.write(k + "\t" + m + "\n")

    def write_strands(self):
        """<out>.strand, a line per line of history.txt in its order: ref id, sub id, + or -, SAME, OPP."""
        with open(self.out + ".strand", "w") as f:
            for k, subs in self.merge_dict.items():
                for m in subs:
                    f.write("%s\t%s\t%s\t%d\t%d\n" % ((k, m) + tuple(self.strands[(k, m)])))

    # -- the files -----------------------------------------------------------------------------------------------------------------------
    def apply(self):
        md = self.merge_dict
        for x in range(len(self.cluster)):
            shutil.rmtree(self.ident(x), ignore_errors=True)
        if self.drop == "T":
            for ref, subs in md.items():
                for sub in subs:
                    if sub not in md:
                        for ext in _EXTS:
                            os.remove(sub + ext)
            return
        # Receiving clusters by size ascending: a ref is larger than its subs, so a cluster that both receives and is merged (a chain
        # P -> Q -> R) has received, and carries its new name, when its own ref takes it.
        moved = {}
        for ref in sorted(md, key=lambda k: int(k.rsplit("_", 1)[1])):
            stem, n = ref.rsplit("_", 1)
            n = int(n)
            for sub in md[ref]:
                cur = moved.get(sub, sub)
                n += int(cur.rsplit("_", 1)[1])
                # orient: a sub on the other strand arrives reverse-complemented as a whole — its file holds what it took itself in its
                # own orientation, so a chain composes
                turn = self.orient and self.strands[(ref, sub)][0] == "-"
                for ext in _EXTS:
                    if turn and ext != ".txt":
                        revcomp_fasta(cur + ext, ref + ext)
                    else:
                        with open(cur + ext, "rb") as fi, open(ref + ext, "ab") as fo:
                            shutil.copyfileobj(fi, fo)
                    os.remove(cur + ext)
            final = stem + "_" + str(n)
            for ext in _EXTS:
                os.rename(ref + ext, final + ext)
            moved[ref] = final

    def run(self):
        t0 = time.time()
        self.load()
        t1 = time.time()
        numbers = self.compare()
        t2 = time.time()
        self.decide(numbers)
        self.write_history()
        if self.both_strands:
            self.write_strands()
        print("start merging...." if self.drop != "T" else "start dropping...")
        self.apply()
        self.stats.update(load_s=t1 - t0, compare_s=t2 - t1, apply_s=time.time() - t2, n_clusters=len(self.cluster),
                          n_merged=sum(len(v) for v in self.merge_dict.values()))
        return self


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Merge (or drop) rare clusters that are close to a larger cluster by average nucleotide identity, on the GPU")
    p.add_argument("-i", "--input", required=True, metavar="<file>", help="cluster.txt of extract_cluster.py (Clusters_fa/ beside it)")
    p.add_argument("-p", "--nproc", type=int, default=1, metavar="<int>", help="accepted for compatibility and ignored")
    p.add_argument("-t", "--threshold", type=int, default=20, metavar="<int>",
                   help="clusters of at most this many sequences try to merge into a larger one. Default: 20. 0: every cluster; 1: none")
    p.add_argument("-d", "--drop", type=str, default="T", metavar="<str>", help="T: drop the rare clusters that have a close larger cluster; anything else: merge them into it. Default: T")
    p.add_argument("-a", "--ani", type=float, default=0.8, metavar="<float>", help="mean identity of the reported pairs a merge needs, as a fraction. Default: 0.8")
    p.add_argument("-o", "--out", type=str, default="history.txt", metavar="<file>", help="output: ref id <tab> merged id per line. Default: history.txt")
    p.add_argument("--sketch-size", type=int, default=ANI_MAX_SKETCH, metavar="<int>", help=f"hashes per sketch, {ANI_MIN_SKETCH}..{ANI_MAX_SKETCH}. Default: {ANI_MAX_SKETCH}")
    p.add_argument("--report-floor", type=float, default=0.7, metavar="<float>", help="a sequence pair below this identity is not reported (as fastANI reports nothing below ~0.7-0.8). Default: 0.7")
    p.add_argument("--both-strands", action="store_true",
                   help="compare on both strands (canonical 12-mers): a rare cluster that is the reverse complement of a larger one's neighbour merges too; "
                        "writes <out>.strand (ref id, sub id, + or -, SAME, OPP per line of the history)")
    p.add_argument("--orient", action="store_true",
                   help="with --both-strands and -d other than T: a cluster merged on the other strand is appended reverse-complemented, so the receiving .fa / .tfa keep one orientation")
    p.add_argument("--device", type=int, default=0, help="GPU ordinal (default 0)")
    args = p.parse_args(argv)
    if args.orient and not args.both_strands:
        p.error("--orient needs --both-strands")
    if args.orient and args.drop == "T":
        p.error("--orient needs a merge: -d other than T")
    if not ANI_MIN_SKETCH <= args.sketch_size <= ANI_MAX_SKETCH:
        p.error(f"--sketch-size must be in {ANI_MIN_SKETCH}..{ANI_MAX_SKETCH}")
    if not 0 <= args.ani <= 1:
        p.error("-a must be in 0..1 (a fraction)")
    if not 0 <= args.report_floor <= 1:
        p.error("--report-floor must be in 0..1")
    return args


def main(argv=None):
    from ._abi import prefer_staged_copies
    prefer_staged_copies()                      # a command line owns its process: see _abi.prefer_staged_copies
    e1 = time.time()
    args = parse_args(argv)                     # exit status 2 on bad flags
    app = merge_clstr(inputfile=args.input, output=args.out, threshold=args.threshold, drop=args.drop, ani=args.ani, nproc=args.nproc,
                      sketch_size=args.sketch_size, report_floor=args.report_floor, device=args.device, both_strands=args.both_strands, orient=args.orient)
    app.run()                                   # SystemExit with a message (status 1) on a missing or empty .tfa or an over-long record
    e2 = time.time()
    print("INFO {} Total times: {}".format(time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(time.time())), round(float(e2 - e1), 2)))
