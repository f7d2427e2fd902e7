"""Greedy minimal primer-set cover — drop-in for scripts/get_Maxprimerset.py
(get_Maxprimerset_V1.3.py, "MS"): clusters sorted by number of candidate pairs, for each cluster
the first pair that forms no 3'-end dimer with the already selected set is taken.

The control flow below restates MS:218-356 (including what the reference actually does after a
back-track in the maximum mode: the outer `for` resumes at the row after the one that failed,
MS:257-277).  The dimer test itself (`dimer_examination`, MS:193-215, quadratic in the size of
the selected set in the reference) runs on the GPU and only over pairs that involve a new
primer (dimer.DimerExaminer).

With -r/--ref (a background FASTA) a pair that passes the dimer test must pass an off-target test too: the products its two
primers give on the background on their own and together with the primers already selected (setscreen.OffTargetExaminer, the rule
at the head of include/mprime_setscreen.h — the intent of get_Maxprimerset_V3.py, which cannot run).  Without -r nothing changes.
"""
from __future__ import annotations

import re
import sys
from optparse import OptionParser

from . import iupac
from ._abi import Library
from .dimer import DimerExaminer
from .setscreen import OffTargetExaminer, RefusedPrimer, load_background, reads_of

OT_COLUMNS = ["#Primer", "Primer_rank", "Primer_F", "Primer_R", "Own", "Cross", "Decision"]
OT_SET_COLUMNS = ["Forward_primer", "Reverse_primer", "Products"]

COLUMNS = ["#Primer", "Primer_rank", "Primer_F", "Primer_R", "PCR_product (Length:Tm:Coverage)",
           "Coverage number with error in top N", "Primer position (representative sequence)"]


def _write_clique(path, rows):
    """pandas' DataFrame.to_csv(sep='\\t', index=False) of the reference's `clique` frame: missing
    values print as empty fields."""
    with open(path, "w") as f:
        f.write("\t".join(COLUMNS) + "\n")
        for r in rows:
            f.write("\t".join("" if r.get(c) is None else str(r[c]) for c in COLUMNS) + "\n")


def _row(primers, r, c):
    p = primers[r]
    return {"#Primer": p[0], "Primer_rank": str(c), "Primer_F": p[c], "Primer_R": p[c + 1],
            "PCR_product (Length:Tm:Coverage)": p[c + 2], "Coverage number with error in top N": p[c + 3],
            "Primer position (representative sequence)": p[c + 4]}


class PrimerSetCover:
    def __init__(self, primers, step, examiner: DimerExaminer, offtarget: OffTargetExaminer | None = None, max_offtarget: int = 0,
                 cross_only: bool = False, lookahead: int = 4):
        self.primers = primers
        self.step = step
        self.ex = examiner
        self.ot = offtarget                    # None: the run without -r
        self.max_offtarget, self.cross_only, self.lookahead = max_offtarget, cross_only, max(1, lookahead)
        self.ot_log = []                       # one row per pair that reached the off-target test, in test order
        self.selected = set()                  # S of the final set
        if offtarget is not None:              # the first K pairs of every cluster in one batch
            offtarget.ensure([p for r in range(len(primers)) for p in self._pair_primers(r, 0, self.lookahead)])

    def _pair_primers(self, r, first, n):
        """the primers of pairs first .. first + n - 1 of cluster r"""
        row, out = self.primers[r], []
        for j in range(first, first + n):
            c = 1 + j * self.step
            if c > len(row) - self.step:
                break
            out += [row[c], row[c + 1]]
        return out

    def _offtarget(self, r, c, selected):
        """True: the pair (r, c), which forms no dimer with the set, is rejected for what it amplifies on the background."""
        if self.ot is None:
            return False
        f, rv = self.primers[r][c], self.primers[r][c + 1]
        if f not in self.ot.ids or rv not in self.ot.ids:        # the walk reached an unscreened pair: the next K of this cluster
            self.ot.ensure(self._pair_primers(r, (c - 1) // self.step, self.lookahead))
        own, cross = self.ot.counts(f, rv, selected)
        bad = (cross if self.cross_only else own + cross) > self.max_offtarget
        self.ot_log.append([self.primers[r][0], str(c), f, rv, str(own), str(cross), "rejected" if bad else "selected"])
        return bad

    def write_offtarget(self, output):
        """<out>.offtarget.tsv (the log) and <out>.offtarget.set.tsv (the ordered pairs of final-set primers with a product)."""
        with open(output + ".offtarget.tsv", "w") as f:
            f.write("\t".join(OT_COLUMNS) + "\n")
            for row in self.ot_log:
                f.write("\t".join(row) + "\n")
        with open(output + ".offtarget.set.tsv", "w") as f:
            f.write("\t".join(OT_SET_COLUMNS) + "\n")
            for a in sorted(self.selected):
                for b in sorted(self.selected):
                    if self.ot.products(a, b):
                        f.write("{}\t{}\t{}\n".format(a, b, self.ot.products(a, b)))

    def _dimer(self, f, r, primer_set):
        return self.ex.any_dimer(iupac.expand(f) + iupac.expand(r), sorted(primer_set))

    @staticmethod
    def _grow(primer_set, f, r):
        return primer_set | set(iupac.expand(f) + iupac.expand(r))

    def maximal(self, output, next_candidate):
        """greedy_maximal_primers (MS:291-356): a cluster whose pairs all dimerise is skipped and
        written to the .next file."""
        primers, step = self.primers, self.step
        primer_set = set()
        selected = set()
        clique = []
        r, c = 0, 1
        while r < len(primers):
            if len(primers[r]) <= 1:
                print("Non primers: virus {} missing!".format(primers[r][0]))
                next_candidate.write("\t".join(primers[r]) + "\n")
                r, c = r + 1, 1
                continue
            while c <= len(primers[r]) - step:
                if self._dimer(primers[r][c], primers[r][c + 1], primer_set) or self._offtarget(r, c, selected):
                    c += step
                    if c > len(primers[r]) - step:
                        clique.append({"#Primer": primers[r][0]})
                        print("virus {} missing!".format(primers[r][0]))
                        next_candidate.write("\t".join(primers[r]) + "\n")
                        r, c = r + 1, 1
                        break
                else:
                    clique.append(_row(primers, r, c))
                    primer_set = self._grow(primer_set, primers[r][c], primers[r][c + 1])
                    selected = selected | {primers[r][c], primers[r][c + 1]}
                    r, c = r + 1, 1
                    break
            else:
                # a row too short to hold one pair never enters the inner loop and never advances in
                # the reference either (it would spin); treat it like an exhausted cluster
                raise ValueError(f"row {r} has {len(primers[r])} fields: not a multiple of step")
        self.selected = selected
        _write_clique(output, clique)

    def maximum(self, output):
        """greedy_primers (MS:218-282): back-track to the previous cluster's next pair when a
        cluster is exhausted; exit(1) when the first cluster is exhausted."""
        primers, step = self.primers, self.step
        primer_set = set()
        selected, saved_selected = set(), {}
        saved_set, jdict = {}, {}
        clique = []
        blank_row = 0
        c = 1
        for row in range(len(primers)):
            r = row
            if len(primers[r]) <= 1:
                blank_row += 1
                continue
            while c <= len(primers[r]) - step:
                if self._dimer(primers[r][c], primers[r][c + 1], primer_set) or self._offtarget(r, c, selected):
                    c += step
                    while c > len(primers[r]) - step:                    # backtrack_to_previous_row, MS:246-255
                        r -= 1
                        if r < blank_row:
                            print("Non maximum primer set. Try maximal primer set!")
                            sys.exit(1)
                        if r not in jdict:
                            # The reference reads jdict[row_pointer] of a cluster it never selected from (a blank cluster, or one
                            # the search already left: the for-loop's row pointer and the back-tracking one diverge) and dies
                            # with KeyError, exit status 1, nothing written (tests/golden/maxset_multi.json.gz, seeds 3 and 7).
                            # Same status here, with a message instead of a traceback.
                            print("KeyError: {} (the maximum-set search cannot back-track past this cluster; "
                                  "the reference script fails here too)".format(r), file=sys.stderr)
                            sys.exit(1)
                        c = jdict[r] + step
                        primer_set = saved_set[r]
                        selected = saved_selected[r]
                        clique.pop()
                else:
                    clique.append(_row(primers, r, c))
                    saved_set[r] = primer_set
                    saved_selected[r] = selected
                    primer_set = self._grow(primer_set, primers[r][c], primers[r][c + 1])
                    selected = selected | {primers[r][c], primers[r][c + 1]}
                    jdict[r] = c
                    c = 1
                    break
        self.selected = selected
        _write_clique(output, clique)


def parse_args(argv=None):
    parser = OptionParser("Usage: %prog -i [input] -o [output] \n Options: {-s [step] -m [T]}", version="%prog 0.0.4")
    parser.add_option("-i", "--input", dest="input", help="Input file: primers")
    parser.add_option("-a", "--adaptor", dest="adaptor", type="str",
                      default="TCTTTCCCTACACGACGCTCTTCCGATCT,TCTTTCCCTACACGACGCTCTTCCGATCT",
                      help="Adaptor sequence (accepted for compatibility; the reference does not use it either)")
    parser.add_option("-s", "--step", dest="step", default=5, type="int",
                      help="distance between primers; column number of primer1_F to primer2_F.")
    parser.add_option("-m", "--method", dest="method", default="T", type="str",
                      help="which method: maximal or maximum. If -m [T] use maximal; else maximum")
    parser.add_option("-o", "--out", dest="out", help="Prefix of out file: candidate primers")
    parser.add_option("--device", dest="device", default=0, type="int", help="GPU ordinal")
    parser.add_option("-r", "--ref", dest="ref", default=None, type="str",
                      help="background FASTA (the sequences themselves, not an index): pairs are also tested for what they amplify on it")
    parser.add_option("-p", "--product", dest="product", default="150,2000", type="str", help="product size range lo,hi: lo < size < hi. Default: 150,2000")
    parser.add_option("-d", "--dist", dest="dist", default=12, type="int", help="length of the 3' term that is mapped; 0: the whole primer. Default: 12")
    parser.add_option("-t", "--tmp", dest="tmp", default=None, type="str", help="accepted for compatibility; nothing is written to it")
    parser.add_option("--seedmms", dest="seedmms", default=1, type="int", help="mismatches a site may have, 0..3. Default: 1")
    parser.add_option("--max-offtarget", dest="max_offtarget", default=0, type="int", help="products a pair may add. Default: 0")
    parser.add_option("--cross-only", dest="cross_only", default=False, action="store_true",
                      help="count only products with an already selected primer (for a background that holds the design targets)")
    parser.add_option("--lookahead", dest="lookahead", default=4, type="int", help="pairs per cluster that are screened at once. Default: 4")
    options, _ = parser.parse_args(argv)
    try:
        lo, hi = (int(x) for x in options.product.split(","))
    except ValueError:
        parser.error("-p/--product takes two integers lo,hi")
    if lo >= hi:
        parser.error("-p/--product: lo must be below hi")
    options.size_lo, options.size_hi = lo, hi
    if options.dist < 0:
        parser.error("-d/--dist must not be negative")
    if not 0 <= options.seedmms <= 3:
        parser.error("--seedmms takes 0..3")
    if options.max_offtarget < 0:
        parser.error("--max-offtarget must not be negative")
    if options.lookahead < 1:
        parser.error("--lookahead must be at least 1")
    if options.input is None:
        parser.print_help()
        print("Input file must be specified !!!")
        sys.exit(1)
    if options.out is None:
        parser.print_help()
        print("No output file provided !!!")
        sys.exit(1)
    return options


def _check_offtarget_input(options):
    """With -r, before a file is written or a kernel launched: the background exists and holds bases, and every candidate primer can be
    screened.  Exit status 1 with the name otherwise.  Returns the background."""
    try:
        background = load_background(options.ref)
        with open(options.input, "r") as f:
            for line in f:
                row = list(filter(None, line.strip().split("\t")))
                for c in range(1, len(row) - options.step + 1, options.step):
                    reads_of(row[c], options.dist)
                    reads_of(row[c + 1], options.dist)
    except (RefusedPrimer, ValueError) as e:
        print(str(e), file=sys.stderr)
        sys.exit(1)
    return background


def run(options, library: Library | None = None, offtarget: OffTargetExaminer | None = None):
    """offtarget: an examiner to use instead of the one -r would build (precomputed pair counts: no device is asked for them)."""
    ref = getattr(options, "ref", None)
    background = _check_offtarget_input(options) if ref and offtarget is None else None
    if re.search("/", options.input):                                        # MS:363-367
        parts = options.input.split("/")
        sort = "/".join(parts[:-1]) + "/sort." + parts[-1]
    else:
        sort = "sort." + options.input
    with open(options.input, "r") as primers_file, open(sort, "w") as f:
        primers = list(sorted([list(filter(None, line.strip().split("\t"))) for line in primers_file], key=len))
        for i in primers:
            f.write("\t".join(i) + "\n")
    lib = library if library is not None else Library()
    ctx = lib.context(options.device)
    if background is not None:
        offtarget = OffTargetExaminer(ctx, background, options.size_lo, options.size_hi, options.dist, options.seedmms)
    if offtarget is None:
        cover = PrimerSetCover(primers, options.step, DimerExaminer(ctx, threshold=3.0))
    else:
        cover = PrimerSetCover(primers, options.step, DimerExaminer(ctx, threshold=3.0), offtarget, getattr(options, "max_offtarget", 0),
                               getattr(options, "cross_only", False), getattr(options, "lookahead", 4))
    if options.method == "T":
        next_candidate = options.out.rstrip(".xls") + ".next.xls"             # MS:375 (strips characters, not a suffix)
        with open(next_candidate, "w") as nxt:
            cover.maximal(options.out, nxt)
    else:
        cover.maximum(options.out)
    if offtarget is not None:
        cover.write_offtarget(options.out)
    return cover


def main(argv=None):
    from ._abi import prefer_staged_copies
    prefer_staged_copies()                      # a command line owns its process: see _abi.prefer_staged_copies
    run(parse_args(argv))


if __name__ == "__main__":
    main()
