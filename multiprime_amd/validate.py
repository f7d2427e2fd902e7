"""Drop-in for scripts/primer_coverage_validation_by_BWT_V9.py ("V9") — SURVEY §8f-3: which primer pairs of a primer set
amplify which sequences of a database when a few mismatches are tolerated.  The reference maps the expanded 3' terms with
bowtie2, splits the SAM by strand with samtools (V9:264-286) and pairs the surviving sites per sequence; here the mapping is
ONE exhaustive GPU scan (mp_kmm_scan, csrc/scan.hip) and the rest is restated in three stages of its own:

  TermTable    the reads: every distinct 3' term of the primer file, expanded (V9:205-239)  ->  <primers>.term.fa
  sites        {strand: {sequence: {start: primer}}} — from the GPU scan, or, exactly as the reference does when it finds them
               (V9:270-271), from existing <primers>.for.sam / .rev.sam files filtered by the MD:Z rule of build_dict (V9:241-262)
  amplicons    per sequence, the (forward start, reverse start) combinations inside the size range (V9:318-345), vectorised
  reports      <out>, <out>.pair.num, <out>.total.acc.num, <out>.unmatched.fa (V9:377-398)

Same class name (`off_targets`), constructor arguments, flags and output files as the reference script.

PARITY: everything around the mapper is pinned to the reference — tests/golden/validate.json.gz holds what the unmodified V9
class writes for hand-written and seeded SAM input (tests/golden/make_golden_validate.py), this module reproduces it from the
same SAM text, and the GPU scan is checked end to end against the same stages fed with the SAM lines its hits stand for.  The
MAPPER: bowtie2 / samtools are not installed in the authoring image, so the mapping step is replaced by its acceptance rule
under default end-to-end scoring — an ungapped alignment with at most floor((0.6 + 0.6 L) / 6) mismatches (minimum score
-0.6 - 0.6 L at 6 per mismatch; `--max-mismatch` overrides), both strands, every site (`-a`).  That rule is pinned to the
reference author's own bowtie2 + samtools run of rule BWT_validation (multiPrime.py:441-457), whose output ships in the reference
tree: all 1158 sequences whose text is available (485 with a product row, 673 without) are decided identically, and the
neighbouring rules (budget 0 / 2, 3'-term threshold 0 / 2) are not (tests/golden/make_golden_bwt.py, tests/test_validate_bwt.py).
Beyond what that run exercises: sites bowtie2's seed heuristics (-N, -L 8) miss are found here, and GAPS are opt-in (`gaps=True`,
`--gaps`).  bowtie2's default scoring charges 5 + 3 g for a gap of g bases on either side and keeps gaps `--gbar 4` bases away from
the read ends, so under the same minimum score an 18-base term may carry a 1- or 2-base indel instead of its mismatch, a 23-base
term a 1-base indel and a mismatch.  With `gaps` a site counts when the ungapped rule holds, or when ONE gap of g <= 4 bases, at
least 4 bases from either end of the read, leaves 6 mm + 5 + 3 g within the penalty ceiling floor(0.6 + 0.6 L) (6 M under
`--max-mismatch M`) and the last `-t` aligned pairs match — the MD:Z reading of sites_of_sam: the run ends at a deletion and passes
over inserted bases (include/mprime_offtarget.h states the rule; csrc/kmm.hpp: kmm_gap_kernel; gap_scan_host below is its host
form).  What remains different with `gaps`: two gaps in one alignment (they fit from L = 26 on) and gaps longer than 4 bases
(from L = 29 on) are not looked for.  Without `gaps` every output is what it was: the recorded run does not tell the two rules
apart (tests/test_gapscan.py), so the default stays ungapped.

Orders the reference takes from a Python set (sequences in <out>, names inside a shared term id, unmatched records) are
deterministic here: first appearance in the forward sites / the primer file / sorted names.
"""
from __future__ import annotations

import os
import sys
import pickle
import re
import time
from pathlib import Path

import numpy as np

from . import iupac
from ._abi import KMM_MAX_GAP, Library
from .dimer import PATTERN_MAX_LEN

_READ_INDEX = re.compile(r"_\d+$")          # a read name ends in the index of its expansion (V9:249)
_MD_TAG = re.compile(r"MD:Z:(\w+)")
_DIGITS = re.compile(r"\d+")


def degenerate_seq(primer: str):
    """Concrete sequences of a degenerate one in itertools.product order (V9:193-203); other characters stay as they are."""
    out = [""]
    for ch in primer:
        out = [a + b for a in out for b in (iupac.MEMBERS[ch] if ch in "RYMKSWHBVDN" else ch)]
    return out


def bowtie2_mismatch_budget(length: int) -> int:
    """Mismatches bowtie2 --end-to-end admits with default scoring: min score -0.6 - 0.6 L, 6 per mismatch (high quality)."""
    return int((0.6 + 0.6 * length) // 6)


def bowtie2_penalty_ceiling(length: int) -> int:
    """floor(0.6 + 0.6 L): what an end-to-end alignment may lose under default scoring (6 per mismatch, 5 + 3 g per gap)."""
    return int(0.6 + 0.6 * length)          # in floating point, as bowtie2_mismatch_budget: ceiling // 6 is that budget at every length


GBAR = 4                                    # bowtie2 --gbar: no gap within 4 bases of either read end
_BASE_CODE = np.full(256, 4, np.uint8)      # A C G T (either case) -> 0..3, everything else 4: matches nothing
for _i, _ch in enumerate("ACGT"):
    _BASE_CODE[ord(_ch)] = _BASE_CODE[ord(_ch.lower())] = _i


def gap_scan_host(data, row_off, reads, max_penalty, max_gap, term):
    """The gapped rule of include/mprime_offtarget.h on the host, vectorised over start positions: hits [n][4] = (sequence, start,
    read, strand) sorted as Context.kmm_scan sorts them.  `reads`: concrete ACGT strings.  The checker of mp_kmm_gap_scan_resident,
    and what scan() uses when the loaded library has no gapped entry (the oracle); sized for fixtures, not for databases."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    row_off = np.ascontiguousarray(row_off, dtype=np.int64)
    n, pen = len(data), int(max_penalty)
    empty = np.empty((0, 4), np.int32)
    if n == 0 or not len(reads):
        return empty
    n_gap = min(int(max_gap), KMM_MAX_GAP, (pen - 5) // 3) if pen >= 8 else 0
    budget = pen // 6
    text = np.concatenate([_BASE_CODE[data], np.full(PATTERN_MAX_LEN + KMM_MAX_GAP, 4, np.uint8)])
    row_of = np.repeat(np.arange(len(row_off) - 1), np.diff(row_off))
    room_all = row_off[row_of + 1] - row_off[0] - np.arange(n)              # bases from a start to the end of its sequence
    found = []
    for r, read in enumerate(reads):
        fwd = _BASE_CODE[np.frombuffer(read.encode(), np.uint8)]
        L = len(fwd)
        if term > L:
            continue
        for strand in (0, 1):
            P = fwd if strand == 0 else (3 - fwd[::-1])
            # columns 0 .. GBAR - 1 pair on diagonal 0 in every alignment: more mismatches there than any form allows end a start
            head = np.zeros(n, np.int32)
            for j in range(min(GBAR, L)):
                head += text[j:j + n] != P[j]
            cand = np.nonzero((head <= budget) & (room_all >= L - n_gap))[0]
            if not len(cand):
                continue
            W = text[cand[:, None] + np.arange(L + n_gap)]
            room = room_all[cand]
            A = W[:, :L] != P
            ok = (A.sum(1) <= budget) & (room >= L) & ~A[:, L - term:].any(1)
            below = np.concatenate([np.zeros((len(cand), 1), np.int32), np.cumsum(A, 1, dtype=np.int32)], 1)     # below[:, c]: A's before c
            for g in range(1, n_gap + 1):
                m = (pen - 5 - 3 * g) // 6
                for kind, cols in (("D", L), ("I", L - g)):
                    B = (W[:, g:g + L] != P) if kind == "D" else (W[:, :cols] != P[g:])
                    above = np.concatenate([np.cumsum(B[:, ::-1], 1, dtype=np.int32)[:, ::-1], np.zeros((len(cand), 1), np.int32)], 1)
                    c = np.arange(GBAR, (min(L - GBAR, L - term) if kind == "D" else cols - GBAR) + 1)
                    if not len(c) or term > cols:
                        continue
                    fits = below[:, c] + above[:, c] <= m
                    first = cols - term                                      # the term columns: first .. cols - 1
                    if kind == "D":                                          # all of them right of the deletion (c <= first)
                        fits &= (above[:, [first]] == 0) & (room >= L + g)[:, None]
                    else:                                                    # right of c from B, left of it from A
                        k = np.maximum(c, first)
                        fits &= (below[:, k] == below[:, [first]]) & (above[:, k] == 0) & (room >= cols)[:, None]
                    ok |= fits.any(1)
            sel = cand[ok]
            if len(sel):
                rows = row_of[sel]
                found.append(np.stack([rows, sel - (row_off[rows] - row_off[0]), np.full(len(sel), r), np.full(len(sel), strand)], 1))
    if not found:
        return empty
    h = np.concatenate(found).astype(np.int32)
    return h[np.lexsort((h[:, 3], h[:, 2], h[:, 1], h[:, 0]))]


class TermTable:
    """The reads of the mapping step: expanded 3' terms -> read name (V9:205-239).  A line of the primer file that starts with
    '>' names the lines after it; every other line is a primer (the reference does not join wrapped records, nor does this)."""

    def __init__(self, primer_file, term_len):
        owners = {}                                  # term -> primer names, file order
        name = None
        with open(primer_file) as f:
            for line in f:
                text = line.strip()
                if line.startswith(">"):
                    name = text.lstrip(">")
                else:
                    owners.setdefault(text if term_len == 0 else text[-term_len:], []).append(name)
        self.reads = {}                              # concrete sequence -> the ids that expand to it
        for term, names in owners.items():
            stem = "_".join(dict.fromkeys(names))
            for j, seq in enumerate(degenerate_seq(term)):
                self.reads.setdefault(seq, []).append(f"{stem}_{j}")

    def names(self):
        return ["_".join(ids) for ids in self.reads.values()]

    def write(self, path):
        with open(path, "w") as fo:
            fo.writelines(f">{name}\n{seq}\n" for seq, name in zip(self.reads, self.names()))


def sites_of_sam(path, threshold):
    """{sequence: {0-based start: primer}} of one strand's SAM file under build_dict's rule (V9:241-262): an alignment counts
    when the number its MD:Z tag ENDS with — read from the tag's last two characters only, so 12 for "5A12" but 0 for "15C10"
    — is at least `threshold`; lines without the tag (unaligned reads) do not count.  Later lines replace earlier ones at the
    same start (the reference turns its list into a dict, V9:320-322)."""
    sites = {}
    with open(path) as f:
        for line in f:
            col = line.strip().split("\t")
            tag = _MD_TAG.search("\t".join(col[11:]))
            if tag and int(_DIGITS.search(tag.group(1)[-2:]).group()) >= threshold:
                sites.setdefault(col[2], {})[int(col[3]) - 1] = _READ_INDEX.split(col[0])[0]
    return sites


def usable_reads(seqs, names):
    """Indices of the reads the scan takes (warning about the others on stderr; a read too long for the scan is an error)."""
    # The reference hands every read to bowtie2, which ignores what it cannot align (an empty read from a blank line of the
    # primer file — V9 get_term keeps it as key "" —, a read with U / I / N left after expansion, a read shorter than a seed).
    # This build does the same: such reads find nothing, with a warning naming them; only when NO read is usable is that an
    # error.  A read BEYOND the packed pattern width is different: bowtie2 would map it, the scan cannot — reporting "no
    # off-target" for a read that was never looked for would be wrong, so that is a hard error naming the read
    # ("Limits": use -l to map the 3' term of longer primers).
    too_long = [names[i] for i, seq in enumerate(seqs) if len(seq) > PATTERN_MAX_LEN]
    if too_long:
        raise ValueError("read(s) longer than the scan's {} bases: {} — map the 3' term instead (-l)".format(
            PATTERN_MAX_LEN, ", ".join(repr(n) for n in too_long[:20]) + (" ..." if len(too_long) > 20 else "")))
    usable = [i for i, seq in enumerate(seqs) if len(seq) >= 4 and not (set(seq.upper()) - set("ACGT"))]
    usable_set = set(usable)
    skipped = [names[i] for i in range(len(seqs)) if i not in usable_set]
    if skipped:
        print("Warning: {} read(s) not scanned (empty, shorter than 4 bases, or not ACGT after expansion), as bowtie2 ignores them: {}".format(
            len(skipped), ", ".join(repr(n) for n in skipped[:20]) + (" ..." if len(skipped) > 20 else "")),
            file=sys.stderr)
    if not usable:
        raise ValueError(f"no usable read: the scan takes 4..{PATTERN_MAX_LEN} bases of ACGT after expansion")
    return usable


def amplicons(forward, reverse, size_lo, size_hi):
    """(start, stop, forward primer, reverse primer, length) of one sequence, in the reference's order (V9:318-345): starts
    ascending, stops ascending, length = stop - start + 1 strictly inside (size_lo, size_hi).  Two quirks are kept: no product
    at all when the sites cannot be closer than size_hi or farther than size_lo as a whole, and the FIRST start without a
    reverse site in [start + size_lo, start + size_hi) ends the search for the later starts as well."""
    starts = np.fromiter(sorted(forward), np.int64, len(forward))
    stops = np.fromiter(sorted(reverse), np.int64, len(reverse))
    if stops[0] - starts[-1] > size_hi or stops[-1] - starts[0] < size_lo:
        return []
    first = np.searchsorted(stops, starts + size_lo, "left")
    last = np.where(starts + size_hi > stops[-1], len(stops) - 1, np.searchsorted(stops, starts + size_hi, "left") - 1)
    dead = np.nonzero(first > last)[0]
    n_live = int(dead[0]) if len(dead) else len(starts)
    # stop - start + 1 < size_hi; from `first` on stop >= start + size_lo, so the lower bound holds already
    last = np.minimum(last, np.searchsorted(stops, starts + size_hi - 1, "left") - 1)
    out = []
    for i in range(n_live):
        a = int(starts[i])
        for b in stops[first[i]:last[i] + 1].tolist():
            if b - a + 1 > size_lo:
                out.append((a, b, forward[a], reverse[b], b - a + 1))
    return out


class off_targets(object):
    def __init__(self, primer_file, term_length, reference_file, PCR_product_size, mismatch_num, outfile, term_threshold,
                 bowtie="bowtie2", nproc=20, targets="None", *, library: Library | None = None, device: int = 0, max_mismatch=None, gaps=False):
        self.bowtie = bowtie                    # accepted for compatibility: no external mapper is run
        self.term_threshold = int(term_threshold)
        self.nproc = nproc
        self.term_len = term_length
        self.primer_file = primer_file
        self.reference_file = reference_file
        self.outfile = outfile
        self.PCR_size = PCR_product_size
        self.mismatch_num = mismatch_num        # bowtie's -N / -n: seed sensitivity only, the scan is exhaustive
        self.targets = targets
        self.max_mismatch = max_mismatch
        self.gaps = bool(gaps)                  # admit bowtie2's one short gap (module docstring); off: the ungapped rule, as ever
        self._library, self._device = library, device
        self.stats = {}

    def _beside_primers(self, suffix):
        return Path(self.primer_file).parent.joinpath(Path(self.primer_file).stem).with_suffix(suffix)

    def penalty_ceiling(self, length):
        """What a read of `length` bases may lose with `gaps`: 6 per mismatch of --max-mismatch, else bowtie2's floor(0.6 + 0.6 L)."""
        return 6 * self.max_mismatch if self.max_mismatch is not None else bowtie2_penalty_ceiling(length)

    # -- sites from the GPU ------------------------------------------------------------------------------------------------
    def scan(self, table: TermTable):
        """Both strands' sites from one exhaustive k-mismatch scan of the reference FASTA (replaces V9:264-316)."""
        from .host import Fasta
        path = str(self.reference_file)
        if not os.path.exists(path):
            raise FileNotFoundError(path + ": the scan needs the reference FASTA itself (a bowtie index prefix is not enough)")
        t0 = time.time()
        fa = Fasta(path)
        data, row_off = fa.rows()
        genes = [s[1:] if s.startswith(">") else s for s in fa.ids]          # a mapper names a sequence by its first token
        seqs, names = list(table.reads), table.names()
        usable = usable_reads(seqs, names)
        lib = self._library if self._library is not None else Library()
        ctx = lib.context(self._device)
        found = []
        try:
            # the database goes to the device ONCE, packed (mp_seq_load: 4 bits per base beside the characters); every mismatch budget
            # scans the stored words (rounds 2-5 sent the ASCII text with every call)
            ctx.seq_load(data, row_off)
            budgets = {}
            for i in usable if self.gaps else ():           # reads by penalty ceiling: one gapped scan each
                budgets.setdefault(self.penalty_ceiling(len(seqs[i])), []).append(i)
            for pen, members in budgets.items():
                if lib.gapscan:
                    codes = iupac.MASK_LUT[np.frombuffer("".join(seqs[i].upper() for i in members).encode(), np.uint8)]
                    off = np.zeros(len(members) + 1, np.int32)
                    np.cumsum([len(seqs[i]) for i in members], out=off[1:])
                    h = ctx.kmm_gap_scan_resident(codes, off, pen, KMM_MAX_GAP, self.term_threshold)
                else:                                       # the oracle library of the CPU tests: the host form of the rule
                    h = gap_scan_host(data, row_off, [seqs[i].upper() for i in members], pen, KMM_MAX_GAP, self.term_threshold)
                if len(h):
                    h = h.copy()
                    h[:, 2] = np.asarray(members, np.int32)[h[:, 2]]
                    found.append(h)
            budgets = {}
            for i in () if self.gaps else usable:
                budgets.setdefault(self.max_mismatch if self.max_mismatch is not None else bowtie2_mismatch_budget(len(seqs[i])), []).append(i)
            for budget, members in budgets.items():
                codes = iupac.MASK_LUT[np.frombuffer("".join(seqs[i].upper() for i in members).encode(), np.uint8)]
                off = np.zeros(len(members) + 1, np.int32)
                np.cumsum([len(seqs[i]) for i in members], out=off[1:])
                h = ctx.kmm_scan_resident(codes, off, budget, self.term_threshold)
                if len(h):
                    h = h.copy()
                    h[:, 2] = np.asarray(members, np.int32)[h[:, 2]]
                    found.append(h)
        finally:
            ctx.close()
        self.stats["scan_s"] = time.time() - t0
        sites = ({}, {})
        if found:
            h = np.concatenate(found)
            h = h[np.lexsort((h[:, 1], h[:, 0], h[:, 2]))]                  # read by read, as a mapper reports them
            primers = [_READ_INDEX.split(n)[0] for n in names]
            for row, pos, read, strand in h.tolist():
                sites[strand].setdefault(genes[row], {})[pos] = primers[read]
        return sites

    # -- reports -------------------------------------------------------------------------------------------------------------
    def _report(self, forward, reverse):
        print("Number of genes with candidate primers: forward ==> {}; reverse ==> {}.".format(len(forward), len(reverse)))
        both = [g for g in forward if g in reverse]
        print("Number of genes with candidate primer pairs: {}.".format(len(both)))
        lo, hi = (int(x) for x in self.PCR_size.split(",")[:2])
        per_pair = {}                                                       # "F<TAB>R" -> [products, {sequences}]
        covered = set()
        with open(self.outfile, "w") as fo:
            fo.write("Chrom (or Genes)\tStart\tStop\tPrimer_F\tPrimer_R\tProduct length\n")
            for gene in both:
                for start, stop, pf, pr, length in amplicons(forward[gene], reverse[gene], lo, hi):
                    fo.write(f"{gene}\t{start}\t{stop}\t{pf}\t{pr}\t{length}\n")
                    tally = per_pair.setdefault(pf + "\t" + pr, [0, set()])
                    tally[0] += 1
                    tally[1].add(gene)
                    covered.add(gene)
        with open(self.outfile + ".pair.num", "w") as fo:
            fo.write("Primer_F\tPrimer_R\tPair_num\ttarget accession number\n")
            for pair, (n, genes) in sorted(per_pair.items(), key=lambda kv: kv[1][0], reverse=True):
                fo.write(f"{pair}\t{n}\t{len(genes)}\n")
        with open(self.outfile + ".total.acc.num", "w") as fo:
            fo.write("total coverage of primer set (PS) is: {}\n".format(len(covered)))
            if self.targets != "None":
                with open(self.targets, "rb") as f:
                    records = pickle.load(f)                                # {name: FASTA record text} (prepare_fa_pickle.py)
                print(len(records), len(covered))
                fo.write("total target number is: {}\n".format(len(records)))
                with open(self.outfile + ".unmatched.fa", "w") as out:
                    out.writelines(records[name] for name in sorted(set(records) - covered))

    def run(self):
        table = TermTable(self.primer_file, self.term_len)
        table.write(self._beside_primers(".term.fa"))
        sams = [self._beside_primers(".for.sam"), self._beside_primers(".rev.sam")]
        if all(p.exists() for p in sams):                                   # V9:270-271: existing SAM files are used, nothing is mapped
            forward, reverse = (sites_of_sam(p, self.term_threshold) for p in sams)
        else:
            forward, reverse = self.scan(table)
        self._report(forward, reverse)


def parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(description="For mismatch coverage stastic (MI355X-native k-mismatch scan instead of bowtie2).")
    p.add_argument("-i", "--input", type=str, required=True, metavar="<file>", help="input file: primer.fa.")
    p.add_argument("-r", "--ref", type=str, required=True, metavar="<str>", help="Reference sequence file (FASTA).")
    p.add_argument("-l", "--len", type=int, default=0, metavar="<int>", help="Length of primer used for mapping (0: whole primer). Default: 0")
    p.add_argument("-t", "--term", type=int, default=4, metavar="<int>", help="Position of mismatch is not allowed in the 3 term of primer. Default: 4")
    p.add_argument("-s", "--size", type=str, default="100,1500", metavar="<str>", help="Length of PCR product, default: 100,1500.")
    p.add_argument("-p", "--proc", type=int, default=20, metavar="<int>", help="Accepted for compatibility (the scan runs on the GPU).")
    p.add_argument("-b", "--bowtie", type=str, default="bowtie2", metavar="<str>", help="Accepted for compatibility: no external mapper is run.")
    p.add_argument("-m", "--seedmms", type=int, default=1, metavar="<int>", help="bowtie seed mismatches: sensitivity only; the scan is exhaustive.")
    p.add_argument("-d", "--dict", type=str, default="None", metavar="<str>", help="Dictionary of targets sequences, binary format (prepare_fa_pickle.py).")
    p.add_argument("-o", "--out", type=str, required=True, metavar="<file>", help="Output file: Prodcut of PCR product with primers.")
    p.add_argument("--max-mismatch", type=int, default=None, help="mismatches per alignment (default: bowtie2's budget floor((0.6 + 0.6 L) / 6))")
    p.add_argument("--gaps", action="store_true", help="also admit bowtie2's one short gap (5 + 3 g for g <= 4 bases, at least 4 bases from "
                                                       "the read ends) within the same minimum score; default: ungapped")
    p.add_argument("--device", type=int, default=0)
    return p.parse_args(argv)


def main(argv=None):
    from ._abi import prefer_staged_copies
    prefer_staged_copies()                      # a command line owns its process: see _abi.prefer_staged_copies
    args = parse_args(argv)
    e1 = time.time()
    off_targets(primer_file=args.input, term_length=args.len, reference_file=args.ref, PCR_product_size=args.size,
                mismatch_num=args.seedmms, outfile=args.out, term_threshold=args.term, bowtie=args.bowtie, nproc=args.proc,
                targets=args.dict, device=args.device, max_mismatch=args.max_mismatch, gaps=args.gaps).run()
    e2 = time.time()
    print("INFO {} Total times: {}".format(time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(time.time())), round(float(e2 - e1), 2)))
