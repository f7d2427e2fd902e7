"""Inputs shared by tests/test_ont.py (CPU), tests/test_ont_gpu.py and tests/golden/make_golden_ont.py: the synthetic sequencing run the
golden file records, and the (pieces, keys) pools the device is compared on.  Everything is drawn from seeded generators."""
import random

import ont_ref as ref

# two of the four primers are degenerate (R, Y: four expansions; W: two)
PRIMERS = (">amp1_F\nACGTTGCAAGCTTGACCA\n"
           ">amp1_R\nGGATCCRTTAGCYAAGTC\n"
           ">amp2_F\nTTGACCGWAACGTCATGG\n"
           ">amp2_R\nCATGCATGCAAGGTTCCAGT\n")
LENGTH = 18


def _dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _damage(rng, s, n):
    """n substitutions or one-base indels."""
    s = list(s)
    for _ in range(n):
        if not s:
            s.append(rng.choice("ACGT"))
            continue
        at = rng.randrange(len(s))
        kind = rng.random()
        if kind < 0.5:
            s[at] = rng.choice([c for c in "ACGT" if c != s[at]])
        elif kind < 0.75:
            del s[at]
        else:
            s.insert(at, rng.choice("ACGT"))
    return "".join(s)


def golden_reads():
    """About 40 reads: amplicons of both primer pairs on both strands with clean and damaged ends, a cross pair, a read shorter than
    the piece length, an unrelated read, a read with N and lower-case letters."""
    rng = random.Random(20221008)
    seqs = [s for rec in PRIMERS.split(">")[1:] for s in [rec.split("\n")[1]]]
    pairs = [(seqs[0], seqs[1])] * 3 + [(seqs[2], seqs[3])] * 2 + [(seqs[0], seqs[3])]
    reads = []
    for i in range(36):
        f, r = pairs[i % len(pairs)]
        f, r = rng.choice(ref.expand(f)), rng.choice(ref.expand(r))
        hits = i % 4                                 # 0: clean ends, then one, two, three defects per end
        amp = _damage(rng, f, hits) + _dna(rng, rng.randint(30, 80)) + ref.rc(_damage(rng, r, hits))
        reads.append(ref.rc(amp) if i % 3 == 2 else amp)
    reads.append("ACGTTGCAAGC")                      # shorter than the piece length
    reads.append(_dna(rng, 90))                      # unrelated
    reads.append("acgttgcaagcttgacca" + _dna(rng, 40) + "GACTTRGCTAANGGATCC")
    reads.append(seqs[2].replace("W", "A") + _dna(rng, 50) + ref.rc(seqs[3]))
    return reads


def fastq_text(reads):
    """Four lines per read; the last line has no newline."""
    return "\n".join("@read%d\n%s\n+\n%s" % (i, s, "I" * len(s)) for i, s in enumerate(reads))


def fasta_text(reads):
    """Two lines per read; the last sequence line has no newline, so its second piece is a whole piece."""
    return "\n".join(">read%d\n%s" % (i, s) for i, s in enumerate(reads))


# ---- the device pools -------------------------------------------------------------------------------------------------------------------
PIECE_COUNTS = (1, 63, 64, 65, 129)                  # lane and wave edges
KEY_COUNTS = (1, 2, 64, 65, 150)
N_PIECES, N_KEYS = 300, 150


def pool():
    """(pieces, keys): 150 keys of 1, 17, 18, 20 and 64 letters (mostly 18 and 20; difflib's time grows with the length), 300 pieces that are near-copies of a key or of
    its shifted end, cut as the tool cuts them — among them pieces of 0, 1, 17 + newline, 18, 63 and 64 bytes, N, lower case."""
    rng = random.Random(7)
    key_len = [18, 1, 17, 20, 64] + [64 if i % 48 == 47 else rng.choice((18, 18, 18, 20, 20, 17)) for i in range(N_KEYS - 5)]
    keys = []
    for n in key_len:
        k = _dna(rng, n)
        while k in keys:
            k = _dna(rng, n)
        keys.append(k)
    fixed = ["", "A", keys[2] + "\n", keys[0], keys[4][:30] + "N" + keys[4][31:63], keys[4], "N" * 18, keys[0].lower(),
             keys[3][:9] + "N" + keys[3][10:18], "\n", keys[0][1:] + "\n", "ACACACACACACACACAC", "A" * 18]
    pieces = list(fixed)
    while len(pieces) < N_PIECES:
        k = keys[rng.randrange(N_KEYS)]
        if rng.random() < 0.15:
            k = _dna(rng, rng.choice((18, 18, 18, 18, 40, 64)))
        s = _damage(rng, k, rng.randint(0, 4)) if k else k
        if rng.random() < 0.3:
            s = s[rng.randint(0, 3):] + _dna(rng, rng.randint(0, 3))
        if rng.random() < 0.3:
            s = s[-17:] + "\n"
        pieces.append(s[:64])
    return pieces, keys


def word_edge():
    """(pieces, keys) at the edge of the kernel form on 32-bit masks: keys of 32, 31, 20 and 1 letters, pieces of 30 .. 32 bytes that are
    near-copies, shifted copies and reversed copies of them (matches on the outermost diagonals), all of at most 32 bytes."""
    rng = random.Random(32)
    keys = [_dna(rng, n) for n in (32, 31, 32, 20, 1, 32, 30, 32)]
    keys += ["A" * 32, "AC" * 16, keys[0][16:] + keys[0][:16]]
    pieces = ["A" * 32, "CA" * 16, "A" * 31 + "\n", keys[0], keys[0][::-1], keys[0][31] + keys[0][:31], keys[2][1:] + "\n", keys[1] + "N"]
    while len(pieces) < 40:
        k = keys[rng.randrange(len(keys))]
        s = _damage(rng, k, rng.randint(0, 5))
        if rng.random() < 0.4:
            s = s[rng.randint(0, 4):] + _dna(rng, rng.randint(0, 4))
        pieces.append(s[:32] if rng.random() < 0.7 else s[-31:] + "\n")
    return pieces, keys


def tie_cases():
    """[(pieces, keys, expected key index per piece, what)]."""
    a = "A" * 10
    return [
        ([a], ["CCCCCCCCCC", "AAAAAACC", "AAAAA", "GGGG"], [1], "equal q, different (M, T): 12/18 and 10/15 both round to 0.67, the first wins"),
        ([a], ["CCCCCCCCCC", "AAAAA", "AAAAAACC", "GGGG"], [1], "the same two the other way round"),
        ([a], ["TTTT", "AAAAAACC", "AAAAAAGG", "AAAAAATT"], [1], "equal (M, T) at three indices"),
        (["", a], ["ACGT", "", "A"], [1, 2], "an empty piece against an empty key is ratio 1.0 (T = 0)"),
        (["NNNN\n", "acgt"], ["ACGT", "TTTT"], [0, 0], "nothing matches: ratio 0 everywhere, the first key"),
    ]
