"""The panel-update rule of include/mprime_panel.h restated plainly on strings and dicts (no numpy, nothing of multiprime_amd): the checker
of multiprime_amd/panel.py and of mp_dimer_cross / mp_amplicon_join_classes / mp_offtarget_classes.  tests/test_panel.py pins it to what
the unmodified reference wrote for the fixtures of tests/golden/panel/."""
import math
import re
from bisect import bisect_left
from itertools import product
from pathlib import Path

MEMBERS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "M": "AC", "K": "GT", "S": "GC", "W": "AT", "H": "ATC", "B": "GTC",
           "V": "GAC", "D": "GAT", "N": "ATGC"}
COMP = str.maketrans("ATGCRYMKSWHBVDN", "TACGYRKMSWDVBHN")
FREE = [[-0.7, -0.81, -0.65, -0.65], [-0.67, -0.72, -0.8, -0.65], [-0.69, -0.87, -0.72, -0.81], [-0.61, -0.69, -0.67, -0.7]]
PEN = [[0.4, 0.575, 0.33, 0.73], [0.23, 0.32, 0.17, 0.33], [0.41, 0.45, 0.32, 0.575], [0.33, 0.41, 0.23, 0.4]]
HB = [[2, 2.5, 2.5, 2], [2.5, 3, 3, 2.5], [2.5, 3, 3, 2.5], [2, 2.5, 2.5, 2]]
INIT = {"A": 2.8, "T": 2.8, "C": 1.82, "G": 1.82}
BIT = {"A": 0, "C": 1, "G": 2, "T": 3}
DIMER_HEADER = ["Primer_ID", "Primer seq", "Primer end", "Delta G", "Primer end length", "End (distance 1)", "End (GC)", "Dimer-primer_ID",
                "Dimer-primer seq", "End (distance 2)", "Loss"]
OFFTARGET_HEADER = ["Chrom (or Genes)", "Start", "Stop", "Primer_F", "Primer_R", "Product length"]
NUM_HEADER = "SeqName\tPrimer_ID\tDimer-primer_ID\tRowSum"


def expand(seq):
    return ["".join(t) for t in product(*(MEMBERS[c] for c in seq))]


def rc(seq):
    return seq.translate(COMP)[::-1]


def loss(l, gc, d1, d2):
    return math.log10((2 ** l * 2 ** gc) / ((d1 + 0.1) * (d2 + 0.1)))


def delta_g(end):
    worst = []
    for s in expand(end):
        g = 0
        for n in range(len(s) - 1):
            i, j = BIT[s[n + 1]], BIT[s[n]]
            g += FREE[i][j] * HB[i][j] + PEN[i][j]
        if end[-2:] == "TA":
            g += INIT[s[0]] + 0.4 + 0.4
        else:
            g += INIT[s[0]] + 0.4
        worst.append(g)
    return round(max(worst), 2)


def parse_primers(path):
    out, name = {}, ""
    for line in open(path):
        if line.startswith(">"):
            name = line.strip()
        else:
            out[line.strip()] = name
    return out


def sets_of(core, new):
    """(seqs laid out [uniq_new | uniq_core | common], merged names, jobs [(x, y_lo, y_hi)], number of core jobs)."""
    uniq_new = [s for s in new if s not in core]
    uniq_core = [s for s in core if s not in new]
    common = [s for s in new if s in core]
    seqs = uniq_new + uniq_core + common
    merged = {}
    for s in uniq_new:
        merged[s] = new[s]
    for s in uniq_core:
        merged[s] = core[s]
    for s in common:
        merged[s] = new[s] + "|" + core[s]
    at = {s: i for i, s in enumerate(seqs)}
    jobs = [(at[s], 0, len(uniq_new)) for s in core] + [(at[s], 0, len(seqs)) for s in new]
    return seqs, merged, jobs, len(core)


def ends_of(primer):
    """[(l, expansion index, end)]: lengths min(t, len) for t = 18 .. 5 longest first, each once; expansion order inside a length."""
    out, seen = [], set()
    for t in range(18, 4, -1):
        l = min(t, len(primer))
        if l in seen:
            continue
        seen.add(l)
        out.extend((l, ei, e) for ei, e in enumerate(expand(primer[-l:])))
    return out


def pair_hit(x, y):
    """The first passing (l, end expansion, y expansion, idx) of the ordered pair x -> y, or None."""
    for l, ei, end in ends_of(x):
        for pi, p in enumerate(expand(y)):
            idx = p.find(rc(end))
            if idx >= 0:
                d2 = len(p) - l - idx
                if loss(l, end.count("G") + end.count("C"), 0, d2) > 3 or delta_g(end) < -5:
                    return (l, ei, pi, idx)
    return None


def cross_records(seqs, jobs):
    """[(job, y, l, end expansion, y expansion, idx)] ordered by (job, y): what mp_dimer_cross returns after sorting."""
    out, memo = [], {}
    for j, (x, y_lo, y_hi) in enumerate(jobs):
        for y in range(y_lo, y_hi):
            k = (seqs[x], seqs[y])
            if k not in memo:
                memo[k] = pair_hit(*k)
            if memo[k]:
                out.append((j, y) + memo[k])
    return out


def dimer_lines(core_path, new_path):
    core, new = parse_primers(core_path), parse_primers(new_path)
    seqs, merged, jobs, n_core = sets_of(core, new)
    lines = []
    for j, y, l, ei, pi, idx in cross_records(seqs, jobs):
        x = seqs[jobs[j][0]]
        end = expand(x[-l:])[ei]
        gc = end.count("G") + end.count("C")
        d2 = len(seqs[y]) - l - idx
        partner = new[seqs[y]] if j < n_core else merged[seqs[y]]
        lines.append("\t".join(map(str, (merged[x], x, end, delta_g(end), l, 0, gc, partner, seqs[y], d2, loss(l, gc, 0, d2)))))
    return lines


def count_lines(lines, left, right):
    """The .dimer_num / .offtargets.num body: per value of column `left`, in order of first appearance, its count there and in `right`."""
    a, b = {}, {}
    for line in lines:
        col = line.split("\t")
        a[col[left]] = a.get(col[left], 0) + 1
        b[col[right]] = b.get(col[right], 0) + 1
    return ["\t".join(map(str, (k, a[k], b.get(k, 0), a[k] + b.get(k, 0)))) for k in a]


# ---- off-targets ---------------------------------------------------------------------------------------------------------------------
def beside(path, suffix):
    return Path(path).parent.joinpath(Path(path).stem).with_suffix(suffix)


def sam_sites(path):
    """{gene: {start: read}} of one SAM file: the last line at a start wins; MD:Z must end (last two characters) in a number >= 5."""
    out = {}
    for line in open(path):
        col = line.strip().split("\t")
        md = re.search(r"MD:Z:(\w+)", "\t".join(col[11:])).group(1)
        if int(re.search(r"[A-Z]?(\d+)", md[-2:]).group(1)) >= 5:
            out.setdefault(col[2], {})[int(col[3]) - 1] = col[0]
    return out


def join(forward, reverse, lo, hi):
    """One sequence: [(start, stop, F, R, length)]."""
    starts, stops = sorted(forward), sorted(reverse)
    if stops[0] - starts[-1] > hi:
        return []
    if stops[-1] - starts[0] < lo:
        return []
    out = []
    for a in starts:
        left = bisect_left(stops, a + lo)
        right = len(stops) - 1 if a + hi > stops[-1] else bisect_left(stops, a + hi) - 1
        if left > right:
            break
        for k in range(left, right + 1):
            n = stops[k] - a + 1
            if n > hi:
                break
            if lo < n < hi:
                out.append((a, stops[k], forward[a], reverse[stops[k]], n))
    return out


JOINS = [(0, 1), (1, 0), (1, 1)]           # (class of the forward sites, class of the reverse sites)


def join_classes(sites, lo, hi):
    """sites: [(class, strand, row, position, read)], any order, the last entry of a (class, strand, row, position) wins.
    [(row, start, stop, F, R, length, join class)] in class order, rows ascending."""
    at = {}
    for cls, strand, row, pos, read in sites:
        at.setdefault((cls, strand), {}).setdefault(row, {})[pos] = read
    out = []
    for k, (fc, rcl) in enumerate(JOINS):
        f, r = at.get((fc, 0), {}), at.get((rcl, 1), {})
        for row in sorted(f):
            if row in r:
                out.extend((row,) + p + (k,) for p in join(f[row], r[row], lo, hi))
    return out


def offtarget_lines(core_path, new_path, lo, hi):
    """(lines of <out>.offtargets without the header, genes in order of first appearance in core.for, core.rev, new.for, new.rev)."""
    files = [[sam_sites(beside(p, s)) for s in (".for.sam", ".rev.sam")] for p in (core_path, new_path)]
    genes = list(dict.fromkeys(g for cls in files for strand in cls for g in strand))
    lines = []
    for fc, rcl in JOINS:
        for g in genes:
            if g in files[fc][0] and g in files[rcl][1]:
                lines.extend("\t".join(map(str, (g,) + p)) for p in join(files[fc][0][g], files[rcl][1][g], lo, hi))
    return lines


def blocks_by_gene(lines):
    """{gene: [lines of the gene, in file order]} per join: a gene may appear in several joins, so the key is (occurrence, gene)."""
    out, seen_run = {}, {}
    prev = None
    for line in lines:
        g = line.split("\t")[0]
        if g != prev:
            seen_run[g] = seen_run.get(g, 0) + 1
            prev = g
        out.setdefault((g, seen_run[g]), []).append(line)
    return out

