"""Inputs of the DegePrime tests (tests/test_dege.py, tests/test_dege_gpu.py) and of tests/golden/make_golden_dege.py: the small
hand-made alignment the trims were recorded from, and the synthetic alignments that reach every edge of csrc/dege.hip.  The sizes at
which the kernels change their path come from the constants multiprime_amd/_abi.py exports."""
from multiprime_amd._abi import DEGE_LDS_LIMIT, DEGE_MERGE_LDS, DEGE_SORT_MIN

LETTERS = "ACGT"

# ---- the small alignment of the recorded trims ---------------------------------------------------------------------------------------------
BASE = "ACGTTGCAAGGCTTACGATCGGATCCAAGTTGACCTGAAGTCCATGGT"          # 48 columns
SPARSE = {8: ("s1", "s4"), 9: ("s1", "s4"), 25: ("s2",), 40: ("s1", "s5"), 41: ("s1", "s5")}       # column: the only rows with a base there


def _sub(s, edits):
    s = list(s)
    for col, ch in edits.items():
        s[col] = ch
    return "".join(s)


def small_alignment():
    """[(id, row)]: '.', lower case, U, sparse columns, IUPAC letters, an inner gap, and a reference row (ref1) that lacks columns the
    others have."""
    rows = [
        ("ref1", _sub(BASE, {30: "-", 31: "-"})),
        ("s1", _sub(BASE, {3: "A"})),
        ("s2", BASE.lower().replace("t", "u")),
        ("s3", "...." + BASE[4:44] + "...."),
        ("s4", _sub(BASE, {15: "G", 33: "T"})),
        ("s5", "--" + _sub(BASE, {20: "C"})[2:]),
        ("s6", ".." + _sub(BASE, {12: "N", 30: "R"})[2:]),
        ("s7", _sub(BASE, {18: "-", 19: "-", 20: "-"})),
        ("s8", "........" + BASE[8:36] + "............"),
        ("s9", _sub(BASE, {28: "C", 44: "A"})),
    ]
    out = []
    for name, row in rows:
        row = list(row)
        for col, holders in SPARSE.items():
            if name not in holders and row[col] != ".":
                row[col] = "-"
        out.append((name, "".join(row)))
    return out


def small_fasta():
    """The rows over two lines each, with a description after the id of one record."""
    return "".join(">%s%s\n%s\n%s\n" % (i, " some description" if i == "s4" else "", r[:30], r[30:]) for i, r in small_alignment())


TRIMS = {                                      # name: TrimAlignment flags
    "default": [],
    "min05": ["-min", "0.5"],
    "min09_trail02": ["-min", "0.9", "-max_trailing", "0.2"],
    "trailgap_min05": ["-trailgap", "-min", "0.5"],
    "ref": ["-ref", "ref1"],
}
SMALL_TABLE = ("min05", ["-l", "6", "-d", "4", "-skip", "2"])         # the Perl table recorded on one of the lower-case outputs
SUB_FLAGS = {"l": 18, "d": 12}                  # dege_sub: DegePrime's defaults otherwise
WIDE_FLAGS = {"l": 18, "d": 24, "skip": 5}      # dege_wide


# ---- synthetic alignments -------------------------------------------------------------------------------------------------------------------
def lcg(seed):
    """A stream of 31-bit integers (the tests must not depend on a library's generator)."""
    x = (seed * 2862933555777941757 + 3037000493) & ((1 << 64) - 1)
    while True:
        x = (x * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
        yield x >> 33


def mer_of(word, l):
    return "".join(LETTERS[(word >> (2 * (l - 1 - p))) & 3] for p in range(l))


def distinct_rows(n, l, seed=1, repeats=()):
    """n rows of width l, each a different gap-free mer (scattered over the 2-bit values), then `repeats[k]` further copies of row k."""
    g = lcg(seed)
    seen, rows = set(), []
    while len(rows) < n:
        w = 0
        for _ in range((2 * l + 15) // 16):
            w = (w << 16) | (next(g) & 0xFFFF)
        w %= 1 << (2 * l)
        if w not in seen:
            seen.add(w)
            rows.append(mer_of(w, l))
    for k, extra in enumerate(repeats):
        rows += [rows[k]] * extra
    return rows


def random_rows(n, width, seed, p_gap=0.0, p_lower=0.0, p_dot=0.0, p_iupac=0.0, n_variants=4, lead=0):
    """n rows of `width` columns drawn around n_variants founder rows with point changes, so that windows hold repeated mers."""
    g = lcg(seed)
    founders = ["".join(LETTERS[next(g) % 4] for _ in range(width)) for _ in range(n_variants)]
    rows = []
    for r in range(n):
        s = list(founders[next(g) % n_variants])
        for c in range(width):
            x = next(g) % 1000
            if x < 30:
                s[c] = LETTERS[next(g) % 4]
            x = next(g) % 1000 / 1000.0
            if x < p_gap:
                s[c] = "-"
            elif x < p_gap + p_lower:
                s[c] = s[c].lower()
            elif x < p_gap + p_lower + p_iupac:
                s[c] = "RYSWKMBDHVN"[next(g) % 11]
        if lead:
            a, b = next(g) % (lead + 1), next(g) % (lead + 1)
            for c in range(a):
                s[c] = "." if next(g) % 1000 / 1000.0 < p_dot else "-"
            for c in range(width - b, width):
                s[c] = "." if next(g) % 1000 / 1000.0 < p_dot else "-"
        rows.append("".join(s))
    return rows


def span_rows(l, skip):
    """Rows whose extents hit and miss the span bounds of window pos = skip + 2 by one, all-gap rows, and rows with inner marks."""
    width = l + 2 * skip + 6
    pos = skip + 2
    body = "".join(LETTERS[(7 * c + c // 3) % 4] for c in range(width))

    def cut(start, end):
        return "-" * start + body[start:end + 1] + "." * (width - end - 1)
    rows = [
        cut(pos - skip, pos + l - 1 + skip),           # both bounds hit exactly
        cut(pos - skip + 1, pos + l - 1 + skip),       # start one too late
        cut(pos - skip, pos + l - 2 + skip),           # end one too early
        cut(pos - skip - 1, pos + l + skip),           # one to spare on both sides
        "-" * width, "." * width,                      # all-gap rows
        cut(0, width - 1),
    ]
    full = cut(0, width - 1)
    last = pos + l - 1
    rows.append(full[:last] + full[last].lower() + full[last + 1:])               # lower case at the last position: the same mer
    rows.append(full[:pos + 1] + full[pos + 1].lower() + full[pos + 2:])          # lower case inside: spans, not gap-free
    rows.append(full[:pos + 1] + "." + full[pos + 2:])                            # '.' inside
    rows.append(full[:pos + 1] + "N" + full[pos + 2:])                            # an IUPAC letter inside
    return rows, pos


WINDOW_ROWS = (1, 63, 64, 65, 257)
WINDOW_L = (2, 16, 17, 31, 32)
# U on both sides of every size at which the window stage changes its path: the sort sizes up to the LDS table's limit, and that limit
SORT_SIZES = [DEGE_SORT_MIN << k for k in range(12) if DEGE_SORT_MIN << k < DEGE_LDS_LIMIT]
UNIQUE_SIZES = sorted({1, DEGE_LDS_LIMIT - 1, DEGE_LDS_LIMIT, DEGE_LDS_LIMIT + 1} | set(SORT_SIZES) | {n + 1 for n in SORT_SIZES})
# U around the 100-draw cap and around the size up to which the merging holds a window in LDS
MERGE_SIZES = (1, 99, 100, 101, DEGE_MERGE_LDS, DEGE_MERGE_LDS + 1)
MERGE_DEGS = (1, 2, 3, 4, 12, 2 ** 20 * 3 ** 5)
MERGE_ITERS = (1, 100, 257)
