"""Drop-in for scripts/primer_specificity.py — SURVEY §8f-3, the off-target half of row 15: which PCR products the primers of a set
could make on a background database (a host genome, a slice of nt) when their 3' terms bind with a few mismatches.  The reference
maps the expanded 3' terms with bowtie2, splits the SAM by strand with samtools and pairs every forward site with the reverse sites
of the same sequence inside the product size range.  Here the stages are those of validate.py (V9), whose script it differs from
only in its defaults and reports:

  reads        validate.TermTable (the expanded 3' terms, `-l` bases each)  ->  <primers>.term.fa
  sites        from existing <primers>.for.sam / .rev.sam files (validate.sites_of_sam: the reference maps nothing when they exist),
               or from the device: mp_offtarget_resident (include/mprime_offtarget.h, csrc/offtarget.hip) scans the database with
               validate's k-mismatch rule, reduces the hits to one primer per site and joins the sites into products on the GPU —
               the host receives products, never hits
  products     validate.amplicons() per sequence (SAM sites), or the device's join (the same rule, tests/test_offtarget_gpu.py)
  reports      <out>, <out>.pair.num, <out>.total.acc.num

What differs from V9, pinned by tests/golden/specificity.json.gz (make_golden_specificity.py, the unmodified reference class on SAM
input): the defaults (-l 18, -t 4, -s 100,1500, -m 1; the class's own: term_length 9, size "150,2000"), the optparse command line,
<out>.total.acc.num without a trailing newline, and no target dictionary (-d) and so no .unmatched.fa.  Sequences come out in the
order of their first forward hit (smallest read, then sequence), where the reference walks a Python set.  `--gaps` (gaps=True)
switches the mapper rule to validate.py's gapped one (mp_offtarget_gap_resident: the same reduction and join behind kmm_gap_kernel).
"""
from __future__ import annotations

import os
import sys
import time
from pathlib import Path

import numpy as np

from . import iupac
from ._abi import KMM_MAX_GAP, Library
from .validate import _READ_INDEX, TermTable, amplicons, bowtie2_mismatch_budget, bowtie2_penalty_ceiling, sites_of_sam, usable_reads


class off_targets(object):
    def __init__(self, primer_file, term_length=9, reference_file="", mismatch_num=1, term_threshold=4, bowtie="",
                 PCR_product_size="150,2000", outfile="", nproc=10, *, library: Library | None = None, device: int = 0,
                 max_mismatch=None, join="device", gaps=False):
        self.bowtie = bowtie                    # accepted for compatibility: no external mapper is run
        self.term_threshold = int(term_threshold)
        self.nproc = nproc
        self.term_len = term_length
        self.primer_file = primer_file
        self.reference_file = reference_file    # the background FASTA itself (the reference turns it into a bowtie index prefix)
        self.outfile = outfile
        self.PCR_size = PCR_product_size
        self.mismatch_num = mismatch_num        # bowtie's -N / -n: seed sensitivity only, the scan is exhaustive
        self.max_mismatch = max_mismatch
        self.gaps = bool(gaps)                  # validate.py's gapped rule (mp_offtarget_gap_resident); off: the ungapped rule
        if join not in ("device", "host"):
            raise ValueError("join is 'device' (the product) or 'host' (validate.py's scan, sites and amplicons(): the check)")
        self.join = join
        self._library, self._device = library, device
        self.stats = {}

    def _beside_primers(self, suffix):
        return Path(self.primer_file).parent.joinpath(Path(self.primer_file).stem).with_suffix(suffix)

    def _size(self):
        lo, hi = (int(x) for x in self.PCR_size.split(",")[:2])
        return lo, hi

    def _counts(self, n_forward, n_reverse, n_both):
        print("Number of genes with candidate primers: forward ==> {}; reverse ==> {}.".format(n_forward, n_reverse))
        print("Number of genes with candidate primer pairs: {}.".format(n_both))

    # -- products from sites (SAM input, and the host path) -----------------------------------------------------------------------
    def products_of_sites(self, forward, reverse):
        self._counts(len(forward), len(reverse), sum(1 for g in forward if g in reverse))
        lo, hi = self._size()
        out = []
        for gene in forward:
            if gene in reverse:
                out.extend((gene,) + p for p in amplicons(forward[gene], reverse[gene], lo, hi))
        return out

    # -- products from the device ---------------------------------------------------------------------------------------------------
    def device_products(self, table: TermTable):
        """The whole screen on the GPU: the background is loaded into the context's store, scanned, reduced and joined there."""
        from .host import Fasta
        path = str(self.reference_file)
        if not os.path.exists(path):
            raise FileNotFoundError(path + ": the scan needs the background FASTA itself (a bowtie index prefix is not enough)")
        t0 = time.time()
        fa = Fasta(path)
        data, row_off = fa.rows()
        genes = [s[1:] if s.startswith(">") else s for s in fa.ids]          # a mapper names a sequence by its first token
        seqs, names = list(table.reads), table.names()
        usable = usable_reads(seqs, names)
        primer_of = [_READ_INDEX.split(names[i])[0] for i in usable]
        primers = list(dict.fromkeys(primer_of))
        ids = {p: k for k, p in enumerate(primers)}
        codes = iupac.MASK_LUT[np.frombuffer("".join(seqs[i].upper() for i in usable).encode(), np.uint8)]
        off = np.zeros(len(usable) + 1, np.int32)
        np.cumsum([len(seqs[i]) for i in usable], out=off[1:])
        budget = [self.max_mismatch if self.max_mismatch is not None else bowtie2_mismatch_budget(len(seqs[i])) for i in usable]
        lo, hi = self._size()
        self.stats["load_s"] = time.time() - t0
        lib = self._library if self._library is not None else Library()
        ctx = lib.context(self._device)
        try:
            t1 = time.time()
            ctx.seq_load(data, row_off)
            t2 = time.time()
            if self.gaps:
                pen = [6 * self.max_mismatch if self.max_mismatch is not None else bowtie2_penalty_ceiling(len(seqs[i])) for i in usable]
                prod = ctx.offtarget_gap_resident(codes, off, np.array([ids[p] for p in primer_of], np.int32), np.array(pen, np.int32),
                                                  KMM_MAX_GAP, self.term_threshold, lo, hi)
            else:
                prod = ctx.offtarget_resident(codes, off, np.array([ids[p] for p in primer_of], np.int32), np.array(budget, np.int32),
                                              self.term_threshold, lo, hi)
            t3 = time.time()
            ms, counts = ctx.offtarget_stats()
        finally:
            ctx.close()
        self.stats.update(seq_load_s=t2 - t1, device_s=t3 - t2, **ms, **counts)
        self._counts(counts["forward_genes"], counts["reverse_genes"], counts["both_genes"])
        return [(genes[r], a, b, primers[f], primers[v], n) for r, a, b, f, v, n in prod.tolist()]

    def host_products(self, table: TermTable):
        """The check of the device path: validate.py's scan (hits to the host, sorted, dicts) and amplicons() per sequence."""
        from . import validate
        t0 = time.time()
        forward, reverse = validate.off_targets(self.primer_file, self.term_len, self.reference_file, self.PCR_size, self.mismatch_num,
                                                self.outfile, self.term_threshold, library=self._library, device=self._device,
                                                max_mismatch=self.max_mismatch, gaps=self.gaps).scan(table)
        t1 = time.time()
        out = self.products_of_sites(forward, reverse)
        self.stats.update(host_sites_s=t1 - t0, host_join_s=time.time() - t1)
        return out

    # -- reports ------------------------------------------------------------------------------------------------------------------------
    def report(self, products):
        per_pair = {}                                                       # "F<TAB>R" -> [products, {sequences}]
        covered = set()
        with open(self.outfile, "w") as fo:
            fo.write("Chrom (or Genes)\tStart\tStop\tPrimer_F\tPrimer_R\tProduct length\n")
            fo.writelines(f"{gene}\t{start}\t{stop}\t{pf}\t{pr}\t{length}\n" for gene, start, stop, pf, pr, length in products)
        for gene, _, _, pf, pr, _ in products:
            tally = per_pair.setdefault(pf + "\t" + pr, [0, set()])
            tally[0] += 1
            tally[1].add(gene)
            covered.add(gene)
        with open(self.outfile + ".pair.num", "w") as fo:
            fo.write("Primer_F\tPrimer_R\tPair_num\ttarget accession number\n")
            for pair, (n, genes) in sorted(per_pair.items(), key=lambda kv: kv[1][0], reverse=True):
                fo.write(f"{pair}\t{n}\t{len(genes)}\n")
        with open(self.outfile + ".total.acc.num", "w") as fo:
            fo.write("total coverage of primer set (PS) is: {}".format(len(covered)))

    def run(self):
        t0 = time.time()
        table = TermTable(self.primer_file, self.term_len)
        table.write(self._beside_primers(".term.fa"))
        sams = [self._beside_primers(".for.sam"), self._beside_primers(".rev.sam")]
        if all(p.exists() for p in sams):                                   # existing SAM files are used, nothing is mapped
            products = self.products_of_sites(*(sites_of_sam(p, self.term_threshold) for p in sams))
        elif self.join == "host":
            products = self.host_products(table)
        else:
            products = self.device_products(table)
        t1 = time.time()
        self.report(products)
        self.stats.update(products_s=t1 - t0, report_s=time.time() - t1, run_s=time.time() - t0, n_products=len(products))


def make_parser():
    """The reference's optparse command line (same options, defaults and destinations), plus --max-mismatch, --gaps and --device."""
    from optparse import OptionParser
    parser = OptionParser('Usage: %prog -i [input] -r [reference fasta] -l [150,2000] -p [10]-o [output]', version="%prog 0.0.6")
    parser.add_option('-i', '--input', dest='input_file', help='input file: primer.fa.')
    parser.add_option('-r', '--ref', dest='ref', help='reference file. fasta format.')
    parser.add_option('-l', '--len', dest='len', default=18, type="int", help='Length of primer, which is used for mapping. Default: 18')
    parser.add_option('-t', '--term', dest='term', default=4, type="int",
                      help='Position of mismatch is not allowed in the 3 term of primer. Default: 4')
    parser.add_option('-s', '--s', dest='size', default="100,1500", type="str", help='Length of PCR product, default: 100,1500.')
    parser.add_option('-p', '--proc', dest='proc', default="20", type="int", help='Accepted for compatibility (the scan runs on the GPU).')
    parser.add_option('-b', '--bowtie', dest='bowtie', default="bowtie2", type="string",
                      help='Accepted for compatibility: no external mapper is run.')
    parser.add_option('-m', '--seedmms', dest='seedmms', default="1", type="int",
                      help='bowtie seed mismatches: sensitivity only, the scan is exhaustive.')
    parser.add_option('-o', '--out', dest='out', help='Prodcut of PCR product with primers.')
    parser.add_option('--max-mismatch', dest='max_mismatch', default=None, type="int",
                      help="mismatches per alignment (default: bowtie2's budget floor((0.6 + 0.6 L) / 6))")
    parser.add_option('--gaps', dest='gaps', default=False, action="store_true",
                      help="also admit bowtie2's one short gap (5 + 3 g for g <= 4 bases, at least 4 bases from the read ends) within the "
                           "same minimum score; default: ungapped")
    parser.add_option('--device', dest='device', default=0, type="int")
    return parser


def parse_args(argv=None):
    """(options, args) as the reference's argsParse() returns them, with its checks (help and exit 1 when a required one is missing)."""
    argv = sys.argv[1:] if argv is None else list(argv)
    parser = make_parser()
    options, args = parser.parse_args(argv)
    if not argv:
        parser.print_help()
        sys.exit(1)
    for value, what in ((options.input_file, "Input file must be specified !!!"), (options.ref, "reference (fasta) must be specified !!!"),
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
    off_targets(primer_file=options.input_file, term_length=options.len, reference_file=options.ref, PCR_product_size=options.size,
                mismatch_num=options.seedmms, outfile=options.out, term_threshold=options.term, bowtie=options.bowtie, nproc=options.proc,
                device=options.device, max_mismatch=options.max_mismatch, gaps=options.gaps).run()
    e2 = time.time()
    print("INFO {} Total times: {}".format(time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(time.time())), round(float(e2 - e1), 2)))
