"""Inputs of the panel-update tests (tests/test_panel.py, tests/test_panel_gpu.py): primer lists with their jobs, sized as small as the
kernel's paths allow, built from a seeded generator so that the CPU and the GPU suites see the same strings."""
import numpy as np

COMP = str.maketrans("ACGT", "TGCA")
LENGTHS = (3, 4, 5, 17, 18, 19, 31, 32, 33, 64)      # around the shortest end, the 18-base end, the staged table and the plane width


def rc(s):
    return s.translate(COMP)[::-1]


def random_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def all_against_all(n):
    return [(x, 0, n) for x in range(n)]


def length_set(long=True):
    """Primers of every boundary length, each planted so that its 3' end pairs somewhere in a partner of every other length: x of
    length a ends in RC of a stretch of the partner of length b.  long=False keeps the lengths up to 32 (32-bit planes)."""
    rng = np.random.default_rng(11)
    lengths = [n for n in LENGTHS if long or n <= 32]
    hosts = [random_seq(rng, n) for n in lengths]
    seqs = list(hosts)
    for h in hosts:                                   # a primer per host whose end pairs at the host's 5' start, one at its 3' end
        for where in (0, 1):
            k = min(len(h), 9 if where == 0 else 20)         # the 3' plants reach the longest end, 18
            piece = h[:k] if where == 0 else h[-k:]
            for n in lengths:
                body = random_seq(rng, max(n - k, 0))
                seqs.append((body + rc(piece))[-n:] if n >= k else rc(piece)[-n:])
    seqs = list(dict.fromkeys(seqs))
    return seqs, all_against_all(len(seqs))


def degenerate_set():
    """Degenerate letters on either side: an end whose two expansions BOTH occur in the partner (the first in expansion order must be
    reported), a degenerate partner whose second expansion is the one that pairs, a degenerate letter outside every end."""
    host = "TTAGGCATCCGTAACGT" + "GCATCAGT" + "AA" + "GCATTAGT" + "CC"      # holds RC of ...ACTGATGC and of ...ACTAATGC
    x_both = "GGATTCAAGTCA" + "ACTRATGC"                                    # R = A/G: ACTAATGC and ACTGATGC both pair with host
    y_deg = "CCGGATATAGG" + "GCATYAGT" + "TT"                               # Y = C/T: both expansions pair with x_both's two ends
    x_far = "NACGGTCAATTGCCATAGCAAGGTCA"                                    # N at position 0 of 26: no end holds it
    y_far = rc(x_far[-10:]) + "ACCA"
    x_three = "TTGACCAGTTACAGGBCATG"                                        # B = G/T/C inside the shorter ends only
    y_three = "AA" + rc("GGTCATG") + "CCTTAACC"
    seqs = [host, x_both, y_deg, x_far, y_far, x_three, y_three, "ACGTNNACGTACGTTGCAAGGCC", "GGCCTTGCAACGTACGTNNACGT"]
    return seqs, all_against_all(len(seqs))


def range_set():
    """600 primers, every third one pairing with primer 0's end; jobs whose ranges start and stop inside a 256-partner stride, an
    empty range, a range of one, the whole list, and the three panel layouts (no core, no new, everything common)."""
    rng = np.random.default_rng(12)
    x = random_seq(rng, 22)
    seqs = [x]
    for i in range(1, 600):
        body = random_seq(rng, 20)
        seqs.append(body + rc(x[-8:]) + "A" * (i % 4) if i % 3 == 0 else body)
    n = len(seqs)
    jobs = [(0, 0, n), (0, 0, 0), (0, 5, 6), (0, 3, 259), (0, 250, 262), (0, 255, 257), (0, 256, 512), (0, 257, 600), (0, 511, 513),
            (3, 590, 600), (7, 0, 300), (0, n, n)]
    return seqs, jobs


def drain_set(every):
    """One job against 1300 partners of which every `every`-th holds RC of the job's 8-base end at its 3' end (every = 1: all of them):
    more than one flush of the LDS hit buffer, and a last queue that is partly filled."""
    rng = np.random.default_rng(13 + every)
    x = "ATTGCACTAGGCTATCGGACTGAC"
    end = rc(x[-8:])
    seqs = [x]
    while len(seqs) < 1301:
        body = random_seq(rng, 14, "AT")              # A/T bodies cannot hold the G/C-rich end by chance
        s = body + end if (len(seqs) - 1) % every == 0 else body + "TTATATAT"
        if s not in seqs:
            seqs.append(s)
    return seqs, [(0, 1, 1301)]


def dg_only_pair():
    """x's 7-base end GCGCATT pairs at the 5' start of a 30-base partner: d2 = 23, Loss 2.95 <= 3, deltaG -7.74 < -5."""
    x = "ATTACATTCAATA" + "GCGCATT"
    y = rc("GCGCATT") + "ATATTAATTATATTTAATATTAT"
    return [x, y], [(0, 1, 2)]


def background_case():
    """(rows, core primers, new primers): a store of four rows of a few hundred bases with planted sites of 20-base primers — a primer
    read forward (strand 0), its reverse complement (strand 1), a copy with one mismatch at its 5' side (found with one mismatch
    allowed) and a copy with a mismatch among its last five bases (never found); products in all three join classes on row 0, a
    position claimed by a core and a new primer alike (the primers share their last 9 bases), a reverse site whose 9-base term needs its one
    mismatch."""
    rng = np.random.default_rng(14)
    core = [("cF", "ATGGCTAGCTTAGGACCTGA"), ("cR", "TTGACCATGCAAGTCCGATG")]
    new = [("nF", "CAGTTACGGATCCATAGCAA"), ("nR", "GGATACCTTGAGCAATCGTA"), ("nF2", "TTACGCATTAGAGGACCTGA")]   # nF2 ends like cF
    by = dict(core + new)

    def mutate(s, at):
        return s[:at] + ("A" if s[at] != "A" else "C") + s[at + 1:]
    rows = []
    for plan in ([(10, "cF", 0), (40, "nF", 0), (150, "nR", 1), (210, "cR", 1), (260, "nR", 1)],
                 [(5, mutate(by["nF"], 2), 0), (120, "cR", 1), (200, mutate(by["cF"], 18), 0), (250, "nR", 1)],
                 [(30, "cF", 0), (60, "nF2", 0), (200, mutate(by["cR"], 18), 1), (300, "nF", 0)],
                 [(0, "nF", 0), (100, rc(mutate(by["nR"], 1)), 0), (330, "cR", 1)]):
        text = list(random_seq(rng, 350, "AT"))                  # A/T filler: no primer (each holds G and C in its last five) binds by chance
        for pos, what, strand in plan:
            s = by.get(what, what)
            s = rc(s) if strand else s
            text[pos:pos + len(s)] = s
        rows.append("".join(text))
    return rows, core, new
