"""Drop-in for scripts/Primer_set_update.py ("PU"): screen NEW primers against a validated CORE set — which new primers form 3'-end
dimers with the panel (`-f D`), and which core/new or new/new combinations of 3' terms amplify something in a background (`-f O`).
include/mprime_panel.h states the rule; tests/panel_ref.py restates it plainly; tests/golden/panel/ holds what the unmodified reference
writes for small inputs.

  Dimer         the rectangular search of PU:258-294 on the GPU (mp_dimer_cross: a job per primer, its partners a range of the list
                [uniq_new | uniq_core | common]); the floating-point columns of the few hits are recomputed on the host with the
                reference's expressions.  The two decisions inside the search — Loss > 3 and round(deltaG, 2) < -5 — reach the device as an
                exact byte table and exact double constants that are only added, as in dimer.py.
  off_targets   reads = the expanded 3' terms of each file (<stem>.term.fa, written when absent); sites from seeded
                <stem>.sam/.for.sam/.rev.sam triplets (PU:324-351: nothing is mapped then) or from this build's mapper, the ungapped
                k-mismatch scan of the background FASTA (`-m` mismatches, 5 matching bases at the 3' end, both strands); three joins by
                origin (core F x new R, new F x core R, new F x new R) on the device (mp_offtarget_classes / mp_amplicon_join_classes).

Each class has a host path (`search="host"`, `join="host"`) that restates the same rule in Python over the same inputs: the check of the
device path, and what the CPU suite runs.  It is chosen by the caller, never fallen back to.

Departures from PU, both documented in INTEGRATION.md: the mapper is not bowtie 1 (its -n/-l/-e --best --strata policy cannot be run
here), and the .primer_set / .gene_position caches the reference pickles beside its inputs are neither read nor written.  Orders the
reference takes from a process pool or a Python set are fixed here: dimer lines in job order, then partner order (uniq_new in new-file
order, uniq_core in core-file order, common in new-file order); off-target sequences per join class in store order (SAM input: order of
first appearance in core.for, core.rev, new.for, new.rev).
"""
from __future__ import annotations

import math
import os
import re
import sys
import time
from bisect import bisect_left
from collections import defaultdict
from pathlib import Path

import numpy as np

from . import iupac
from ._abi import Library
from .dimer import HEADERS, MAX_LEN, PATTERN_MAX_LEN, dg_limit, encode_primers
from .thermo import _DG

LOSS_THRESHOLD = 3                         # PU:276, strict
DG_THRESHOLD = -5
TERM_MATCH = 5                             # PU:344: the MD:Z tag must end in a run of at least 5
_ADJUST_INITIATION = {"A": 2.8, "T": 2.8, "C": 1.82, "G": 1.82}     # PU:133
_ADJUST_TA = 0.4
_SYMMETRY = 0.4
_IDX = {"A": 0, "C": 1, "G": 2, "T": 3}
_MD_TAG = re.compile(r"MD:Z:(\w+)")
_MD_LAST = re.compile(r"[A-Z]?(\d+)")
_IUPAC = set("ACGTRYMKSWHBVDN")


# ---- the two floating-point expressions, as the reference writes them ----------------------------------------------------------------
def penalty_points(length: int, gc: int, d1: int, d2: int) -> float:
    """PU:151-152 (not finDimer's 2**d - 0.9 form)."""
    return math.log10((2 ** length * 2 ** gc) / ((d1 + 0.1) * (d2 + 0.1)))


def delta_g(seq: str) -> float:
    """PU:205-218: stack terms, then one term initiation[first] (+ TA) + symmetry; max over expansions, rounded to 2 decimals."""
    ends_ta = seq[-2:] == "TA"
    best = None
    for s in iupac.expand(seq):
        g = 0
        for n in range(len(s) - 1):
            g += _DG[_IDX[s[n + 1]]][_IDX[s[n]]]
        if ends_ta:
            g += _ADJUST_INITIATION[s[0]] + _ADJUST_TA + _SYMMETRY
        else:
            g += _ADJUST_INITIATION[s[0]] + _SYMMETRY
        if best is None or g > best:
            best = g
    return round(best, 2)


def loss_table() -> np.ndarray:
    """loss_hit[l][GC][d2] = Penalty_points(l, GC, 0, d2) > 3, every entry from the reference's expression (the value depends on l + GC
    and d2 only: 2**l * 2**GC is the integer 2**(l + GC))."""
    by_sum = np.array([[penalty_points(sm, 0, 0, d2) > LOSS_THRESHOLD for d2 in range(64)] for sm in range(2 * MAX_LEN + 1)], np.uint8)
    t = np.zeros((MAX_LEN + 1, MAX_LEN + 1, 64), np.uint8)
    for l in range(1, MAX_LEN + 1):
        t[l, : l + 1] = by_sum[l: 2 * l + 1]
    return t


def dg_params() -> np.ndarray:
    """PU's deltaG in the layout of mp_dimer_scan: its one closing term in every [first][last][TA] slot, zeros for Na+ and symmetry."""
    p = np.zeros(16 + 32 + MAX_LEN + 1 + 1, np.float64)
    for i in range(4):
        for j in range(4):
            p[i * 4 + j] = _DG[i][j]
    for a, ca in enumerate("ACGT"):
        for b in range(4):
            p[16 + (a * 4 + b) * 2 + 0] = _ADJUST_INITIATION[ca] + _SYMMETRY
            p[16 + (a * 4 + b) * 2 + 1] = _ADJUST_INITIATION[ca] + _ADJUST_TA + _SYMMETRY
    return p


_TABLES = {}


def tables():
    if not _TABLES:
        _TABLES.update(loss=loss_table(), dg=dg_params(), limit=dg_limit())
    return _TABLES["loss"], _TABLES["dg"], _TABLES["limit"]


# ---- primer files and sets ------------------------------------------------------------------------------------------------------------
def parse_primers(path) -> dict:
    """PU:228-234: {sequence: name line}; a repeated sequence keeps its first position and its last name.  No .primer_set cache."""
    primers, name = {}, ""
    with open(path, "r") as f:
        for line in f:
            if line.startswith(">"):
                name = line.strip()
            else:
                primers[line.strip()] = name
    return primers


def check_primers(primers: dict, path) -> None:
    for seq in primers:
        if not 1 <= len(seq) <= MAX_LEN:
            raise ValueError(f"{path}: primer of {len(seq)} bases (1..{MAX_LEN} supported by this build, see INTEGRATION.md): {seq!r}")
        bad = set(seq) - _IUPAC
        if bad:
            raise ValueError(f"{path}: primer {seq!r} holds {''.join(sorted(bad))!r}: only upper-case IUPAC nucleotide codes are searched")


class PanelSets:
    """PU:179-192 with a fixed order: the list [uniq_new | uniq_core | common] and the names of `merged`."""

    def __init__(self, core: dict, new: dict):
        self.core, self.new = core, new
        self.uniq_new = [s for s in new if s not in core]
        self.uniq_core = [s for s in core if s not in new]
        self.common = [s for s in new if s in core]
        self.seqs = self.uniq_new + self.uniq_core + self.common
        self.index = {s: i for i, s in enumerate(self.seqs)}
        self.merged = {s: new[s] for s in self.uniq_new}
        self.merged.update((s, core[s]) for s in self.uniq_core)
        self.merged.update((s, new[s] + "|" + core[s]) for s in self.common)

    def jobs(self):
        """[(x, y_lo, y_hi)]: core sequences against uniq_new, then new sequences against merged (PU:291-294)."""
        n_new, n = len(self.uniq_new), len(self.seqs)
        return [(self.index[s], 0, n_new) for s in self.core] + [(self.index[s], 0, n) for s in self.new]

    def partner_name(self, job_is_core: bool, y: int) -> str:
        return self.new[self.seqs[y]] if job_is_core else self.merged[self.seqs[y]]


def end_lengths(n: int):
    """PU:195-202: suffix lengths min(t, n) for t = 18 .. 5, each once, longest first."""
    return sorted({min(t, n) for t in range(5, 19)}, reverse=True)


def host_cross(seqs, jobs):
    """The search of mp_dimer_cross in Python: records (job, y, l, end expansion, y expansion, idx), ordered by (job, y)."""
    comp = str.maketrans("ACGT", "TGCA")
    expansions = {}
    dg_hit = {}
    out = []
    for j, (x, y_lo, y_hi) in enumerate(jobs):
        px = seqs[x]
        ends = [(l, ei, e, e.translate(comp)[::-1]) for l in end_lengths(len(px)) for ei, e in enumerate(iupac.expand(px[-l:]))]
        for y in range(y_lo, y_hi):
            py = seqs[y]
            if py not in expansions:
                expansions[py] = iupac.expand(py)
            found = None
            for l, ei, e, rc in ends:
                for pi, p in enumerate(expansions[py]):
                    idx = p.find(rc)
                    if idx < 0:
                        continue
                    d2 = len(p) - l - idx
                    if e not in dg_hit:
                        dg_hit[e] = delta_g(e) < DG_THRESHOLD
                    if penalty_points(l, e.count("G") + e.count("C"), 0, d2) > LOSS_THRESHOLD or dg_hit[e]:
                        found = (j, y, l, ei, pi, idx)
                        break
                if found:
                    break
            if found:
                out.append(found)
    return out


class Dimer(object):
    """Drop-in for PU's class of the same name (PU:247-319).  search: "device" (mp_dimer_cross, the product) or "host" (the check)."""

    def __init__(self, core_primer_file, new_primer_set, outfile, nproc=10, *, library: Library | None = None, device: int = 0,
                 search: str = "device"):
        if search not in ("device", "host"):
            raise ValueError("search is 'device' (the product) or 'host' (the same rule in Python: the check)")
        self.nproc = nproc                      # accepted for compatibility; the search runs on the GPU
        self.core_primer_file = core_primer_file
        self.new_primer_set = new_primer_set
        self.core_primer = parse_primers(core_primer_file)
        self.new_primer = parse_primers(new_primer_set)
        check_primers(self.core_primer, core_primer_file)
        check_primers(self.new_primer, new_primer_set)
        self.outfile = os.path.abspath(outfile)
        self.search = search
        self._library, self._device = library, device
        self.stats = {}

    def scan(self):
        """Hit rows in job order, then partner order, formatted as PU:277-278."""
        sets = PanelSets(self.core_primer, self.new_primer)
        jobs = sets.jobs()
        t0 = time.time()
        if self.search == "host":
            hits = host_cross(sets.seqs, jobs)
        elif not sets.seqs or not jobs:
            hits = []
        else:
            codes, off = encode_primers(sets.seqs)
            loss, dg, limit = tables()
            lib = self._library if self._library is not None else Library()
            ctx = lib.context(self._device)
            try:
                hits = ctx.dimer_cross(codes, off, np.array(jobs, np.int32), loss, dg, limit).tolist()
            finally:
                ctx.close()
        self.stats.update(search_s=time.time() - t0, jobs=len(jobs), primers=len(sets.seqs), hits=len(hits))
        n_core_jobs = len(self.core_primer)
        rows = []
        for j, y, l, ei, pi, idx in hits:
            px, py = sets.seqs[jobs[j][0]], sets.seqs[y]
            end = iupac.expand(px[-l:])[ei]
            d2 = len(py) - l - idx
            gc = end.count("G") + end.count("C")
            rows.append((sets.merged[px], px, end, delta_g(end), l, 0, gc, sets.partner_name(j < n_core_jobs, y), py, d2,
                         penalty_points(l, gc, 0, d2)))
        return rows

    def run(self):
        rows = self.scan()
        primer_id_sum = defaultdict(int)
        dimer_primer_id_sum = defaultdict(int)
        with open(self.outfile, "w") as fo:                                   # PU:298-309
            fo.write("\t".join(HEADERS) + "\n")
            for res in rows:
                primer_id_sum[res[0]] += 1
                dimer_primer_id_sum[res[7]] += 1
                fo.write("\t".join(map(str, res)) + "\n")
        with open(self.outfile + ".dimer_num", "w") as fno:                   # PU:312-318
            fno.write("SeqName\tPrimer_ID\tDimer-primer_ID\tRowSum\n")
            for k in primer_id_sum.keys():
                p_id = primer_id_sum[k]
                d_id = dimer_primer_id_sum[k]
                fno.write("\t".join(map(str, [k, p_id, d_id, p_id + d_id])) + "\n")


# ---- off-target prediction ------------------------------------------------------------------------------------------------------------
def beside(path, suffix):
    """PU:355, 380, 411-415: <parent>/<stem> with its suffix replaced."""
    return Path(path).parent.joinpath(Path(path).stem).with_suffix(suffix)


def term_reads(path, term_len: int):
    """PU:384-408: [(read name line, sequence)] — the last `term_len` bases of every sequence line (0: the whole line) grouped by term,
    the terms expanded, the ids of one concrete sequence joined with '|'."""
    owners, name = {}, ""
    with open(path, "r") as f:
        for line in f:
            if line.startswith(">"):
                name = line.strip()
            else:
                owners.setdefault(line.strip()[-term_len:], []).append(name)
    reads = {}
    for term, names in owners.items():
        stem = "|".join(names)
        for j, seq in enumerate(iupac.expand(term) if set(term) <= _IUPAC else [term]):
            reads.setdefault(seq, []).append(stem + "_" + str(j))
    return [("|".join(ids), seq) for seq, ids in reads.items()]


def read_term_fa(path):
    """[(read name, sequence)] of a .term.fa file: a mapper names a read by the first token after '>'."""
    out, name = [], ""
    with open(path, "r") as f:
        for line in f:
            if line.startswith(">"):
                name = (line[1:].split() or [""])[0]
            elif line.strip():
                out.append((name, line.strip()))
    return out


def sam_sites(path):
    """PU:331-347 of one strand's SAM text: {gene: [[start, read], ...]} in file order — gene = column 3, start = column 4 - 1; a line
    counts when the number found in the last two characters of its MD:Z value is at least 5.  (validate.sites_of_sam(path, 5) applies
    the same MD:Z test but strips the read's expansion index and skips lines without a tag; PU keeps the read name and has no such
    lines after samtools view -F/-f 16 of mapped reads.  Lines without the tag are skipped here too.)"""
    sites = {}
    with open(path, "r") as f:
        for line in f:
            col = line.strip().split("\t")
            if len(col) < 12:
                continue
            tag = _MD_TAG.search("\t".join(col[11:]))
            if not tag:
                continue
            last = _MD_LAST.search(tag.group(1)[-2:])
            if last and int(last.group(1)) >= TERM_MATCH:
                sites.setdefault(col[2], []).append([int(col[3]) - 1, col[0]])
    return sites


def closest(stops, lo_value, hi_value):
    """PU:169-176."""
    left = bisect_left(stops, lo_value)
    right = len(stops) - 1 if hi_value > stops[-1] else bisect_left(stops, hi_value) - 1
    return left, right


def pcr_products(forward: dict, reverse: dict, lo: int, hi: int):
    """PU:427-454 for one sequence: forward / reverse = {position: read}; [(start, stop, read F, read R, length)]."""
    starts, stops = sorted(forward), sorted(reverse)
    if stops[0] - starts[-1] > hi or stops[-1] - starts[0] < lo:
        return []
    out = []
    for a in starts:
        left, right = closest(stops, a + lo, a + hi)
        if left > right:
            break
        for b in stops[left: right + 1]:
            length = b - a + 1
            if length > hi:
                break
            if lo < length < hi:
                out.append((a, b, forward[a], reverse[b], length))
    return out


JOINS = ((0, 1), (1, 0), (1, 1))            # (class of the forward sites, class of the reverse sites): core F x new R, new F x core R, new F x new R


def host_joins(sites, genes, lo, hi):
    """sites[class][strand] = {gene: {position: read}}; products [(gene, start, stop, F, R, length)] in join class, then gene order."""
    out = []
    for fc, rc in JOINS:
        f, r = sites[fc][0], sites[rc][1]
        for gene in genes:
            if gene in f and gene in r:
                out.extend((gene,) + p for p in pcr_products(f[gene], r[gene], lo, hi))
    return out


class off_targets(object):
    """Drop-in for PU's class of the same name (PU:366-506).  join: "device" (the product) or "host" (the same rule in Python)."""

    def __init__(self, core_primer_file, new_primer_set, mismatch_num=1, term_length=9, reference_file="", PCR_product_size="150,2000",
                 outfile="", nproc=10, *, library: Library | None = None, device: int = 0, join: str = "device"):
        if join not in ("device", "host"):
            raise ValueError("join is 'device' (the product) or 'host' (the same rule in Python: the check)")
        self.nproc = nproc                      # accepted for compatibility
        self.term_len = int(term_length)
        self.mismatch_num = int(mismatch_num)
        self.core_primer_file = core_primer_file
        self.new_primer_set = new_primer_set
        self.reference_file = reference_file    # the background FASTA itself (the reference takes a bowtie index prefix)
        self.outfile = outfile
        self.PCR_size = PCR_product_size
        self.join = join
        self._library, self._device = library, device
        self.stats = {}

    def _size(self):
        lo, hi = (int(x) for x in self.PCR_size.split(",")[:2])
        return lo, hi

    def _seeded(self, path):
        return all(beside(path, s).exists() for s in (".sam", ".for.sam", ".rev.sam"))

    def get_term(self, path):
        out = beside(path, ".term.fa")
        if not out.exists():                                                  # PU:381-382: an existing file is left alone
            with open(out, "w") as fo:
                for name, seq in term_reads(path, self.term_len):
                    fo.write(name + "\n" + seq + "\n")
        return read_term_fa(out)

    def check(self):
        """Everything that can be refused is refused before a file is written or a kernel launched."""
        if not 0 <= self.mismatch_num <= 3:
            raise ValueError(f"-m {self.mismatch_num}: the seed mismatches are 0..3")
        if self.term_len < 0:
            raise ValueError(f"-l {self.term_len}: the term length is 0 (whole primer) or positive")
        files = (self.core_primer_file, self.new_primer_set)
        for path in files:
            check_primers(parse_primers(path), path)
        for path in files:
            if self._seeded(path):
                continue
            reads = read_term_fa(beside(path, ".term.fa")) if beside(path, ".term.fa").exists() else \
                [(n[1:], s) for n, s in term_reads(path, self.term_len)]
            for name, seq in reads:
                if len(seq) < 4:
                    raise ValueError(f"{path}: read {name!r} has {len(seq)} bases after -l {self.term_len}: the scan takes 4..{PATTERN_MAX_LEN}")
                if len(seq) > PATTERN_MAX_LEN or set(seq) - set("ACGT"):
                    raise ValueError(f"{path}: read {name!r} is not 4..{PATTERN_MAX_LEN} bases of ACGT after expansion")
            if not self.reference_file:
                raise ValueError(f"-f O needs -r (the background FASTA) unless {beside(path, '.sam')}, .for.sam and .rev.sam exist")
            if not os.path.exists(str(self.reference_file)):
                raise FileNotFoundError(str(self.reference_file) + ": the scan needs the background FASTA itself (a bowtie index prefix is not enough)")

    # -- sites ------------------------------------------------------------------------------------------------------------------------
    def _background(self):
        from .host import Fasta
        fa = Fasta(str(self.reference_file))
        data, row_off = fa.rows()
        return data, row_off, [s[1:] if s.startswith(">") else s for s in fa.ids]

    @staticmethod
    def _encode(seqs):
        codes = iupac.MASK_LUT[np.frombuffer("".join(seqs).encode(), np.uint8)]
        off = np.zeros(len(seqs) + 1, np.int32)
        np.cumsum([len(s) for s in seqs], out=off[1:])
        return codes, off

    def _context(self):
        lib = self._library if self._library is not None else Library()
        return lib.context(self._device)

    def scan_sites(self, reads, background):
        """Both strands' sites of one file from the k-mismatch scan: ({gene: [[start, read]]}, same for the reverse strand), hits read by
        read as a mapper reports them."""
        data, row_off, genes = background
        codes, off = self._encode([s for _, s in reads])
        ctx = self._context()
        try:
            ctx.seq_load(data, row_off)
            h = ctx.kmm_scan_resident(codes, off, self.mismatch_num, TERM_MATCH)
        finally:
            ctx.close()
        sites = ({}, {})
        if len(h):
            h = h[np.lexsort((h[:, 1], h[:, 0], h[:, 2]))]
            for row, pos, read, strand in h.tolist():
                sites[strand].setdefault(genes[row], []).append([pos, reads[read][0]])
        return sites

    def device_screen(self, reads, background):
        """Neither file seeded: scan, site reduction and the three joins on the device (mp_offtarget_classes)."""
        data, row_off, genes = background
        all_reads = [(n, s, 0) for n, s in reads[0]] + [(n, s, 1) for n, s in reads[1]]
        codes, off = self._encode([s for _, s, _ in all_reads])
        lo, hi = self._size()
        ctx = self._context()
        try:
            t0 = time.time()
            ctx.seq_load(data, row_off)
            t1 = time.time()
            prod = ctx.offtarget_classes(codes, off, np.arange(len(all_reads), dtype=np.int32), np.array([c for _, _, c in all_reads], np.int32),
                                         self.mismatch_num, TERM_MATCH, lo, hi)
            t2 = time.time()
            ms, counts = ctx.offtarget_stats()
        finally:
            ctx.close()
        self.stats.update(seq_load_s=t1 - t0, device_s=t2 - t1, **ms, **counts)
        return [(genes[r], a, b, all_reads[f][0], all_reads[v][0], n) for r, a, b, f, v, n, _ in prod.tolist()]

    def device_joins(self, sites, genes, lo, hi):
        """The three joins on the device from resolved sites (mp_amplicon_join_classes)."""
        row = {g: i for i, g in enumerate(genes)}
        names, ids, recs = [], {}, []
        for cls in (0, 1):
            for strand in (0, 1):
                for gene, at in sites[cls][strand].items():
                    for pos, read in at.items():
                        if read not in ids:
                            ids[read] = len(names)
                            names.append(read)
                        recs.append((cls, strand, row[gene], pos, ids[read]))
        recs.sort()
        ctx = self._context()
        try:
            prod = ctx.amplicon_join_classes(np.array(recs, np.int32).reshape(-1, 5), lo, hi)
            ms, counts = ctx.offtarget_stats()
        finally:
            ctx.close()
        self.stats.update(**ms, **counts)
        return [(genes[r], a, b, names[f], names[v], n) for r, a, b, f, v, n, _ in prod.tolist()]

    def products(self):
        files = (self.core_primer_file, self.new_primer_set)
        reads = [self.get_term(p) for p in files]
        seeded = [self._seeded(p) for p in files]
        lo, hi = self._size()
        background = None if all(seeded) else self._background()
        if not any(seeded) and self.join == "device":
            return self.device_screen(reads, background)
        raw = []
        for path, rd, sd in zip(files, reads, seeded):
            raw.append(tuple(sam_sites(beside(path, s)) for s in (".for.sam", ".rev.sam")) if sd else self.scan_sites(rd, background))
            print("Number of genes with candidate primers ({}): forward ==> {}; reverse ==> {}.".format(path, len(raw[-1][0]), len(raw[-1][1])))
        # one read per site: a dict of the list, the last line wins (PU:429-431)
        sites = [[{g: dict(v) for g, v in strand.items()} for strand in cls] for cls in raw]
        if background is not None:
            genes = background[2]
        else:
            genes = list(dict.fromkeys(g for cls in raw for strand in cls for g in strand))
        for label, (fc, rc) in zip(("coreF_new_R", "coreR_new_F", "newF_new_R"), JOINS):
            print("Number of genes with candidate primer pairs of {}: {}.".format(label, sum(1 for g in sites[fc][0] if g in sites[rc][1])))
        if self.join == "device":
            return self.device_joins(sites, genes, lo, hi)
        return host_joins(sites, genes, lo, hi)

    def run(self):
        self.check()
        t0 = time.time()
        products = self.products()
        self.stats.update(products_s=time.time() - t0, n_products=len(products))
        primer_forward_id = defaultdict(int)
        primer_reverse_id = defaultdict(int)
        with open(self.outfile, "w") as fo:                                   # PU:486-496
            fo.write("\t".join(["Chrom (or Genes)", "Start", "Stop", "Primer_F", "Primer_R", "Product length"]) + "\n")
            for res in products:
                primer_forward_id[res[3]] += 1
                primer_reverse_id[res[4]] += 1
                fo.write("\t".join(map(str, res)) + "\n")
        with open(self.outfile + ".num", "w") as fo:                          # PU:499-505
            fo.write("SeqName\tPrimer_ID\tDimer-primer_ID\tRowSum\n")
            for k in primer_forward_id.keys():
                p_id = primer_forward_id[k]
                d_id = primer_reverse_id[k]
                fo.write("\t".join(map(str, [k, p_id, d_id, p_id + d_id])) + "\n")


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def make_parser():
    """PU:34-82: the reference's optparse command line (same options, defaults and destinations), plus --device."""
    from optparse import OptionParser
    parser = OptionParser('Usage: %prog -c core_primer_set -n new_primer_set -r bowtie index '
                          '-s 150,2000 -l 9 -p 10 -m 1 -f DO -o output}', version="%prog 0.0.2")
    parser.add_option('-c', '--core', dest='core', help='core primer file: core_primers.fa. Only fasta is accepted.')
    parser.add_option('-n', '--new', dest='new', help='new primer file: new_primers.fa. Only fasta is accepted.')
    parser.add_option('-r', '--ref', dest='ref', help='reference file: the background FASTA itself (no bowtie index is used).')
    parser.add_option('-s', '--size', dest='size', default="150,2000", help='Length of PCR product, default: [150,2000].')
    parser.add_option('-l', '--len', dest='len', default="9", type="int",
                      help='Length of primer-end, which is used for off-targets prediction.Default: 9; with 0, full length will be used')
    parser.add_option('-m', '--seedmms', dest='seedmms', default="1", type="int", help='Mismatches in seed (can be 0 - 3, default: -n 1).')
    parser.add_option('-p', '--proc', dest='proc', default="10", type="int", help='Accepted for compatibility (the work runs on the GPU).')
    parser.add_option('-f', '--func', dest='func', default="DO", type="str",
                      help='D means finDimer; O means off-targets prediction. Default: DO.'
                           'Use D or O if you want to use fin[D]imer or predict [O]ff-targets.')
    parser.add_option('-o', '--out', dest='out', help='Prefix of out file: candidate primers')
    parser.add_option('--device', dest='device', default=0, type="int")
    return parser


def parse_args(argv=None):
    """(options, args) with PU:85-103's checks: help and exit status 1 when nothing, -c, -n or -o is given."""
    argv = sys.argv[1:] if argv is None else list(argv)
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if not argv:
        parser.print_help()
        sys.exit(1)
    for value, what in ((options.core, "Core primer file must be specified !!!"), (options.new, "New primer file must be specified !!!"),
                        (options.out, "No output file provided !!!")):
        if value is None:
            parser.print_help()
            print(what)
            sys.exit(1)
    return options, args


def main(argv=None):
    from ._abi import prefer_staged_copies
    prefer_staged_copies()                      # a command line owns its process: see _abi.prefer_staged_copies
    e1 = time.time()
    options, _ = parse_args(argv)
    want_d, want_o = re.search("D", options.func), re.search("O", options.func)
    screen = None
    if want_o:                                  # refused before the dimer step launches anything
        screen = off_targets(core_primer_file=options.core, new_primer_set=options.new, term_length=options.len, reference_file=options.ref,
                             PCR_product_size=options.size, outfile=options.out + ".offtargets", mismatch_num=options.seedmms,
                             nproc=options.proc, device=options.device)
        screen.check()
    if want_d:
        print("INFO: Start finDimer ...")
        Dimer(core_primer_file=options.core, new_primer_set=options.new, outfile=options.out + ".dimer", nproc=options.proc,
              device=options.device).run()
    if want_o:
        print("INFO: Start host (human: T2T pre-mRNA) off-targets prediction ...")
        screen.run()
    e2 = time.time()
    print("INFO {} Total time: {}".format(time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(time.time())), round(float(e2 - e1), 2)))
