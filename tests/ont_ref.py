"""The plain-Python yardstick of the read-to-primer assignment (include/mprime_ont.h, multiprime_amd/ontprimer.py): the reference
pipeline restated with difflib itself, and — separately — the integer rule M(a, b) the device runs.  Nothing here imports the package."""
import difflib
import gzip
from itertools import product

BASES = {"R": "AG", "Y": "CT", "M": "AC", "K": "GT", "S": "GC", "W": "AT", "H": "ATC", "B": "GTC", "V": "GAC", "D": "GAT", "N": "ATGC"}
COMPLEMENT = str.maketrans("ACGTRYMKSWHBVDN", "TGCAYRKMSWDVBHN")


def rc(seq):
    return seq.translate(COMPLEMENT)[::-1]


def expand(seq):
    """Every expansion of a degenerate sequence, the leftmost degenerate position slowest."""
    return ["".join(t) for t in product(*[BASES.get(ch, ch) for ch in seq])]


def key_dict(primer_text):
    """{key: label} as the reference's dict ends up (first insertion's place, last insertion's label) and the expand file's text."""
    keys, out, label = {}, [], None
    for line in primer_text.splitlines(True):
        if line.startswith(">"):
            label = line.strip()
        else:
            for j, seq in enumerate(expand(line.strip())):
                out.append("%s | %d\n%s\n" % (label, j, seq))
                keys[seq] = "%s | %d" % (label, j)
                keys[rc(seq)] = "%s | %d" % (label, j)
    return keys, "".join(out)


def pieces(path, fmt, length):
    """[first piece, second piece] per read, as the reference cuts them (a plain file's lines keep their newline)."""
    step = {"fq": 4, "fa": 2}[fmt]
    out = []
    if path.endswith("gz"):
        with gzip.open(path, "rb") as f:
            lines = [x.decode().strip() for x in f.readlines()]
    else:
        with open(path, "r") as f:
            lines = f.readlines()
    for idx, line in enumerate(lines):
        if idx % step == 1:
            out.append([line[:length], line[-length:]])
    return out


def ratio(a, b):
    return round(difflib.SequenceMatcher(None, a, b).ratio(), 2)


def best(piece, keys):
    """(index, ratio) of the first key that reaches the highest rounded ratio."""
    ratios = [ratio(piece, k) for k in keys]
    top = max(ratios)
    return ratios.index(top), top


def name_of(piece, keys, labels, min_ident, full_label=False):
    idx, top = best(piece, keys)
    if top > min_ident:
        return labels[idx] if full_label else labels[idx].split(" | ")[0]
    return "NA"


def order(counts):
    """The .num lines of {pair: count}: count descending, the pair string ascending among equals."""
    return ["Primer_F\tPrimer_R\tNumber\n"] + ["%s\t%d\n" % (p, n) for p, n in sorted(counts.items(), key=lambda x: (-x[1], x[0]))]


def order_lines(lines):
    """Recorded .num lines with ties put into this project's order (the reference's is set-iteration order)."""
    rows = [x.rstrip("\n").rsplit("\t", 1) for x in lines[1:]]
    return [lines[0]] + ["%s\t%s\n" % (p, n) for p, n in sorted(rows, key=lambda x: (-int(x[1]), x[0]))]


def pipeline(path, primer_text, fmt="fq", length=18, min_ident=0.6, full_label=False):
    """The .num lines for one input file."""
    kd, _ = key_dict(primer_text)
    keys, labels = list(kd), list(kd.values())
    counts = {}
    for pair in pieces(path, fmt, length):
        names = sorted(name_of(p, keys, labels, min_ident, full_label) for p in pair)
        counts["\t".join(names)] = counts.get("\t".join(names), 0) + 1
    return order(counts)


# ---- the integer rule -----------------------------------------------------------------------------------------------------------------------
def longest(a, alo, ahi, b, blo, bhi):
    """(i, j, k) of the longest common substring inside the range: the smallest i among equals, then the smallest j.  run[j] is the
    length of the common run that starts at (i, j) and stays inside the range; i and j go downwards, so an equal run found later starts
    earlier and replaces the one kept."""
    bi, bj, bk = alo, blo, 0
    below = [0] * (bhi + 1)
    for i in range(ahi - 1, alo - 1, -1):
        run = [0] * (bhi + 1)
        for j in range(bhi - 1, blo - 1, -1):
            if a[i] == b[j]:
                run[j] = below[j + 1] + 1
                if run[j] >= bk:
                    bi, bj, bk = i, j, run[j]
        below = run
    return bi, bj, bk


def match_count(a, b):
    """M(a, b): the rule of include/mprime_ont.h, written out."""
    m, stack = 0, [(0, len(a), 0, len(b))] if a and b else []
    while stack:
        alo, ahi, blo, bhi = stack.pop()
        i, j, k = longest(a, alo, ahi, b, blo, bhi)
        if k:
            m += k
            if alo < i and blo < j:
                stack.append((alo, i, blo, j))
            if i + k < ahi and j + k < bhi:
                stack.append((i + k, ahi, j + k, bhi))
    return m


def difflib_count(a, b):
    return sum(x.size for x in difflib.SequenceMatcher(None, a, b).get_matching_blocks())


def matrix(pieces, keys):
    """(rounded ratio, match count) of every (piece, key) by difflib, one matcher with the key's index kept across the pieces."""
    sm = difflib.SequenceMatcher(None)
    ratios = [[0.0] * len(keys) for _ in pieces]
    counts = [[0] * len(keys) for _ in pieces]
    for j, k in enumerate(keys):
        sm.set_seq2(k)
        for i, p in enumerate(pieces):
            sm.set_seq1(p)
            ratios[i][j] = round(sm.ratio(), 2)
            counts[i][j] = sum(x.size for x in sm.get_matching_blocks())
    return ratios, counts


def winner(piece, keys, q):
    """(key index, M) by the integer order: the larger q[T][M], the smaller index among equals."""
    top, at = None, None
    for i, k in enumerate(keys):
        m = match_count(piece, k)
        r = q[len(piece) + len(k)][m]
        if top is None or r > top:
            top, at = r, (i, m)
    return at


def winner_difflib(piece, keys):
    """(key index, M) by difflib and Python's round alone."""
    idx, _ = best(piece, keys)
    return idx, difflib_count(piece, keys[idx])
