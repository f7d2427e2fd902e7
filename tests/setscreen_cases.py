"""Planted backgrounds and candidate files for the set screen, shared by the CPU tests (tests/test_setscreen.py), the GPU tests
(tests/test_setscreen_gpu.py) and the recorded fixture (tests/golden/make_golden_setscreen.py).  Everything is seeded."""
import numpy as np

COMP = str.maketrans("ACGT", "TGCA")
DIST = 12


def rc(s):
    return s.translate(COMP)[::-1]


def rnd(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def plant(rows, row, pos, s):
    rows[row] = rows[row][:pos] + s + rows[row][pos + len(s):]


def plant_forward(rows, row, pos, primer, dist=DIST):
    """a forward site of the primer's term at (row, pos)"""
    plant(rows, row, pos, primer[-dist:] if dist else primer)


def plant_reverse(rows, row, pos, primer, dist=DIST):
    """a reverse-strand site of the primer's term at (row, pos): the text reads its reverse complement"""
    plant(rows, row, pos, rc(primer[-dist:] if dist else primer))


def candidate_text(clusters):
    """clusters: [(name, [(F, R), ...])] -> the candidate file of get_Maxprimerset (step 5)"""
    lines = []
    for name, pairs in clusters:
        row = [name]
        for i, (f, r) in enumerate(pairs):
            row += [f, r, "300:60.0:1", str(10 - i), "100:400"]
        lines.append("\t".join(row) + "\n")
    return "".join(lines)


def fasta_text(rows):
    return "".join(">bg{}\n{}\n".format(i, s) for i, s in enumerate(rows))


def all_primers(clusters):
    return list(dict.fromkeys(p for _, pairs in clusters for pair in pairs for p in pair))


def golden_case(seed=11):
    """Four clusters on three background records (products of 150 < length < 2000):
       c0   one clean pair (F0 has a lone forward site): selected
       c3   one pair with a product of its own: rejected, the cluster is exhausted
       c1   pair a: R1a has a reverse site 400 bases behind F0's: rejected by `cross` once F0 is in S; pair b (a degenerate R): selected
       c2   pair a: a product of its own; pair b reuses F0, already in S: selected"""
    rng = np.random.default_rng(seed)
    rows = [rnd(rng, 1200), rnd(rng, 1100), rnd(rng, 900)]
    p = [rnd(rng, 20) for _ in range(12)]
    f0, r0, f3, r3, f1a, r1a, f1b, r1b, f2a, r2a, r2b = p[:11]
    r1b = r1b[:14] + "R" + r1b[15:]
    clusters = [("c1", [(f1a, r1a), (f1b, r1b)]), ("c0", [(f0, r0)]), ("c2", [(f2a, r2a), (f0, r2b)]), ("c3", [(f3, r3)])]
    plant_forward(rows, 0, 100, f0)
    plant_reverse(rows, 0, 500, r1a)
    plant_forward(rows, 1, 200, f2a)
    plant_reverse(rows, 1, 700, r2a)
    plant_forward(rows, 2, 50, f3)
    plant_reverse(rows, 2, 450, r3)
    plant_reverse(rows, 2, 600, r3)
    return rows, clusters
