"""The gapped rule of the validation scan (include/mprime_offtarget.h, `--gaps`): validate.gap_scan_host — the host form that serves
libraries without the gapped entry points — against a brute-force enumerator written here, which loops over the alignment type, the
gap length g, the split column c and every start, straight from the rule's definition, and shares no code with the package.

The cases (planted databases, the seeded random database, the brute force itself) are what tests/test_gapscan_gpu.py runs through the
device kernel as well; the random database's truth is computed once per session."""
import functools

import numpy as np
import pytest

from conftest import load_gz_json
from multiprime_amd import iupac
from multiprime_amd.validate import gap_scan_host, off_targets

GBAR = 4
MAX_GAP = 4
_COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(_COMP)[::-1]


# ---- brute force ------------------------------------------------------------------------------------------------------------------------
def _pairs(kind, g, c, L):
    """(read base j, text offset from p) of every aligned pair, j ascending."""
    if kind == "D":
        return [(j, j) for j in range(c)] + [(j, j + g) for j in range(c, L)]
    return [(j, j) for j in range(c)] + [(j, j - g) for j in range(c + g, L)]


def _alignments(L):
    """Every gapped alignment shape of a read of L bases: (kind, g, c, text bases it spans)."""
    out = []
    for g in range(1, MAX_GAP + 1):
        for c in range(GBAR, L - GBAR + 1):
            out.append(("D", g, c, L + g))
        for c in range(GBAR, L - GBAR - g + 1):
            out.append(("I", g, c, L - g))
    return out


def _mismatch(text_base, read_base):
    return text_base not in "ACGT" or text_base != read_base


def _run(T, p, P, kind, g, c):
    """Matching pairs counted from the read's last base downwards: ends at a mismatch, ends at a deletion, passes over inserted bases."""
    run = 0
    for j, o in reversed(_pairs(kind, g, c, len(P))):
        if (kind == "D" and j < c) or _mismatch(T[p + o], P[j]):
            break
        run += 1
    return run


def brute_min_gap(rows, reads, pen, term):
    """{(row, start, read, strand): the smallest g of an admitted alignment there, 0 for the ungapped rule}.  The mismatch count of one
    alignment shape is taken for every start of a row at once (numpy over p, nothing else); the trailing run is then read base by
    base at the starts whose count fits."""
    best = {}

    def note(key, g):
        if best.get(key, 99) > g:
            best[key] = g
    for r, T in enumerate(rows):
        T = T.upper()
        t = np.frombuffer((T + "#" * 80).encode(), np.uint8)
        bad = ~np.isin(t, np.frombuffer(b"ACGT", np.uint8))
        n = len(T)
        for i, read in enumerate(reads):
            for strand in (0, 1):
                P = read if strand == 0 else rc(read)
                L = len(P)
                pb = np.frombuffer(P.encode(), np.uint8)
                # X[j, d, p]: does read base j mismatch the text base at p + j + d - MAX_GAP ?   (d - MAX_GAP = the diagonal)
                X = np.zeros((L, 2 * MAX_GAP + 1, n), bool)
                for j in range(L):
                    for d in range(-MAX_GAP, MAX_GAP + 1):
                        if j + d >= 0:
                            X[j, d + MAX_GAP] = (t[j + d:j + d + n] != pb[j]) | bad[j + d:j + d + n]
                starts = np.arange(n)
                mm = X[np.arange(L), MAX_GAP].sum(0)
                for p in np.nonzero((mm <= pen // 6) & (starts + L <= n))[0].tolist():
                    run = 0
                    for j in range(L - 1, -1, -1):
                        if _mismatch(T[p + j], P[j]):
                            break
                        run += 1
                    if run >= term:
                        note((r, p, i, strand), 0)
                for kind, g, c, span in _alignments(L):
                    if 5 + 3 * g > pen:
                        continue
                    pairs = _pairs(kind, g, c, L)
                    js = np.array([j for j, _ in pairs])
                    ds = np.array([o - j + MAX_GAP for j, o in pairs])
                    mm = X[js, ds].sum(0)
                    for p in np.nonzero((6 * mm + 5 + 3 * g <= pen) & (starts + span <= n))[0].tolist():
                        if _run(T, p, P, kind, g, c) >= term:
                            note((r, p, i, strand), g)
    return best


def brute_sites(rows, reads, pen, max_gap, term):
    return sorted(k for k, g in brute_min_gap(rows, reads, pen, term).items() if g <= max_gap)


# ---- the scan under test ------------------------------------------------------------------------------------------------------------------
def pack_rows(rows):
    data = np.frombuffer("".join(rows).encode(), np.uint8)
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(x) for x in rows], out=off[1:])
    return data, off


def pack_reads(reads):
    codes = iupac.MASK_LUT[np.frombuffer("".join(reads).encode(), np.uint8)]
    off = np.zeros(len(reads) + 1, np.int32)
    np.cumsum([len(x) for x in reads], out=off[1:])
    return codes, off


def host_sites(rows, reads, pen, max_gap, term):
    data, off = pack_rows(rows)
    return [tuple(x) for x in gap_scan_host(data, off, reads, pen, max_gap, term).tolist()]


# ---- planted cases ------------------------------------------------------------------------------------------------------------------------
def _bases(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def make_read(L, seed=0):
    """A seeded read without two equal neighbours (so that a planted gap has one place to be)."""
    rng = np.random.default_rng(1000 + 31 * L + seed)
    out = [int(rng.integers(0, 4))]
    while len(out) < L:
        b = int(rng.integers(0, 4))
        if b != out[-1] and (len(out) < 2 or b != out[-2]):
            out.append(b)
    return "".join("ACGT"[b] for b in out)


def _other(*bases):
    return next(b for b in "ACGT" if b not in bases)


def site_text(P, kind, g, c, mm=(), fill=None):
    """The text a read P (as the text reads it) aligns to with one gap of g at c, with the text bases of read bases `mm` changed."""
    p = list(P)
    for j in mm:
        p[j] = _other(p[j], p[j - 1] if j else "", p[j + 1] if j + 1 < len(p) else "")
    if kind == "D":
        f = fill if fill is not None else _other(P[c - 1], P[c] if c < len(P) else "") * g
        return "".join(p[:c]) + f + "".join(p[c:])
    return "".join(p[:c]) + "".join(p[c + g:])


def planted_row(site, seed, at=120, tail=100):
    """One row: seeded background, the site at `at`."""
    rng = np.random.default_rng(seed)
    return _bases(rng, at) + site + _bases(rng, tail), at


LENGTHS = (18, 23, 30, 40)


def planted_cases(L):
    """[(name, row text, reads, pen, term, site key (row 0) , expected)] — what the rule's definition says about one planted site each."""
    P = make_read(L)
    mid = L // 2
    cases = []

    def add(name, site, pen, term, want, strand=0, tail=100, read=P):
        row, at = planted_row(site, 7 * len(cases) + L, tail=tail)
        cases.append((name, row, [read], pen, term, (0, at, 0, strand), want))
    for kind in "DI":
        add(f"{kind} pen11 g1", site_text(P, kind, 1, mid), 11, 1, True)
        add(f"{kind} pen11 g1 mm1", site_text(P, kind, 1, mid, mm=(1,)), 11, 1, False)
        add(f"{kind} pen11 g2", site_text(P, kind, 2, mid), 11, 1, True)
        add(f"{kind} pen11 g3", site_text(P, kind, 3, mid), 11, 1, False)
        add(f"{kind} pen14 g1 mm1", site_text(P, kind, 1, mid, mm=(1,)), 14, 1, True)
        add(f"{kind} pen18 g4", site_text(P, kind, 4, mid - (2 if kind == "I" else 0)), 18, 1, True)
        add(f"{kind} pen18 g1 mm2", site_text(P, kind, 1, mid, mm=(1, 5)), 18, 1, False)
        add(f"{kind} term: mismatch in the last 4 columns", site_text(P, kind, 1, mid, mm=(L - 2,)), 14, 4, False)
        add(f"{kind} gap at c = GBAR", site_text(P, kind, 1, GBAR), 11, 1, True)
        add(f"{kind} gap at c = GBAR - 1", site_text(P, kind, 1, GBAR - 1), 11, 1, False)
    add("D gap at c = L - GBAR", site_text(P, "D", 1, L - GBAR), 11, 1, True)
    add("D gap at c = L - GBAR + 1", site_text(P, "D", 1, L - GBAR + 1), 11, 1, False)
    add("I gap at c + g = L - GBAR", site_text(P, "I", 2, L - GBAR - 2), 11, 1, True)
    add("I gap at c + g = L - GBAR + 1", site_text(P, "I", 2, L - GBAR - 1), 11, 1, False)
    add("D term: L - c = term", site_text(P, "D", 1, L - GBAR), 11, 4, True)
    add("D term: L - c < term", site_text(P, "D", 1, L - GBAR), 11, 6, False)
    add("I term: the run crosses the insertion", site_text(P, "I", 1, L - GBAR - 1), 11, 6, True)
    add("D reverse strand", site_text(rc(P), "D", 1, mid), 11, 1, True, strand=1)
    add("I reverse strand", site_text(rc(P), "I", 2, mid), 11, 1, True, strand=1)
    add("D an N among the skipped bases", site_text(P, "D", 2, mid, fill="NN"), 11, 1, True)
    n_site = site_text(P, "D", 1, mid)
    n_site = n_site[:2] + "N" + n_site[3:]
    add("D an aligned N at pen 11", n_site, 11, 1, False)
    add("D an aligned N at pen 14", n_site, 14, 1, True)
    add("D the row ends at p + L + g", site_text(P, "D", 2, mid), 11, 1, True, tail=0)
    add("D the row ends one base earlier", site_text(P, "D", 2, mid)[:-1], 11, 1, False, tail=0)
    add("I the row ends at p + L - g", site_text(P, "I", 2, mid), 11, 1, True, tail=0)
    # a homopolymer: the same site through many c
    H = P[:mid - 3] + _other(P[mid - 4], P[mid + 3]) * 6 + P[mid + 3:]
    add("D inside a homopolymer", H[:mid] + H[mid] + H[mid:], 11, 1, True, read=H)
    add("I inside a homopolymer", H[:mid] + H[mid + 1:], 11, 1, True, read=H)
    # the ungapped rule and a gapped alignment (D, g = 1, c = L - GBAR) at one site: the read ends in a run that the text prolongs
    E = P[:L - GBAR] + _other(P[L - GBAR - 1]) * GBAR
    add("ungapped and gapped at one site", E + E[-1], 11, 1, True, read=E)
    return cases


@functools.lru_cache(maxsize=None)
def planted_truth(L):
    return [brute_sites([row], reads, pen, MAX_GAP, term) for _, row, reads, pen, term, _, _ in planted_cases(L)]


@pytest.mark.parametrize("L", LENGTHS)
def test_planted_sites(L):
    cases, truth = planted_cases(L), planted_truth(L)
    for (name, row, reads, pen, term, key, want), sites in zip(cases, truth):
        assert (key in sites) == want, (L, name, "the brute force disagrees with the case")
        got = host_sites([row], reads, pen, MAX_GAP, term)
        assert got == sites, (L, name)
        assert len(set(got)) == len(got), (L, name, "a site reported twice")
    # the gapped sites are what the flag adds: without gaps none of the gap-only ones is there
    for (name, row, reads, pen, term, key, want) in cases:
        if want and not name.startswith("ungapped"):
            assert key not in host_sites([row], reads, pen, 0, term), (L, name)


def test_planted_g_needs_max_gap():
    """A site that needs g bases is there from max_gap = g on."""
    P = make_read(23)
    for kind in "DI":
        for g in range(1, MAX_GAP + 1):
            row, at = planted_row(site_text(P, kind, g, 9), 50 + g)
            for max_gap in range(MAX_GAP + 1):
                assert ((0, at, 0, 0) in host_sites([row], [P], 18, max_gap, 2)) == (max_gap >= g), (kind, g, max_gap)


# ---- the seeded random database ------------------------------------------------------------------------------------------------------------
RANDOM_PEN, RANDOM_TERM = 18, 3


@functools.lru_cache(maxsize=None)
def random_case():
    """32 rows of 200..3000 bases (a few N among them), 12 reads of 18..40 bases, and per read a dozen copies planted with up to two
    mismatches and / or one indel of 1..4 bases, on either strand — some within the rule, some past it."""
    rng = np.random.default_rng(20240611)
    reads = [make_read(L, seed=k) for k, L in enumerate((18, 18, 19, 20, 21, 22, 23, 23, 24, 26, 30, 40))]
    lens = (200 + 2800 * rng.random(32) ** 3).astype(int)
    lens[0], lens[1] = 200, 3000
    rows = [list(_bases(rng, int(n))) for n in lens]
    for i, read in enumerate(reads):
        for _ in range(12):
            P = read if rng.random() < 0.5 else rc(read)
            mm = tuple(int(x) for x in rng.integers(0, len(P), size=int(rng.integers(0, 3))))
            kind = "DI-"[int(rng.integers(0, 3))]
            if kind == "-":
                site = site_text(P, "D", 0, len(P), mm=mm, fill="")
            else:
                g = int(rng.integers(1, MAX_GAP + 1))
                c = int(rng.integers(GBAR - 1, len(P) - GBAR - (g if kind == "I" else 0) + 2))
                site = site_text(P, kind, g, c, mm=mm)
            row = rows[int(rng.integers(0, 32))]
            at = int(rng.integers(0, max(1, len(row) - len(site) + 1)))
            if rng.random() < 0.15:
                at = max(0, len(row) - len(site))                   # flush with the row's end
            row[at:at + len(site)] = list(site)[:len(row) - at]
    for row in rows[::5]:
        row[int(rng.integers(0, len(row)))] = "N"
    return ["".join(r) for r in rows], reads


@functools.lru_cache(maxsize=None)
def random_truth():
    rows, reads = random_case()
    return brute_min_gap(rows, reads, RANDOM_PEN, RANDOM_TERM)


def test_random_database_equals_brute_force():
    rows, reads = random_case()
    best = random_truth()
    for max_gap in range(MAX_GAP + 1):
        want = sorted(k for k, g in best.items() if g <= max_gap)
        assert host_sites(rows, reads, RANDOM_PEN, max_gap, RANDOM_TERM) == want, max_gap
    by_gap = [sum(1 for g in best.values() if g == k) for k in range(MAX_GAP + 1)]
    assert all(n > 0 for n in by_gap), by_gap                       # every gap length adds sites on this database
    assert len({k[3] for k, g in best.items() if g}) == 2           # on both strands


def test_max_gap_0_is_the_ungapped_scan(oracle_lib):
    """max_gap = 0 against today's kmm_scan (the oracle library's) on the random database, at three ceilings."""
    rows, reads = random_case()
    data, off = pack_rows(rows)
    codes, poff = pack_reads(reads)
    ctx = oracle_lib.context(0)
    try:
        for pen in (11, 18, 6):
            want = ctx.kmm_scan(data, off, codes, poff, pen // 6, RANDOM_TERM)
            assert gap_scan_host(data, off, reads, pen, 0, RANDOM_TERM).tolist() == want.tolist(), pen
            assert len(want)
    finally:
        ctx.close()


# ---- the recorded bowtie2 run ----------------------------------------------------------------------------------------------------------------
def check_bowtie2_fixture_with_gaps(lib, tmp_path):
    from test_validate_bwt import _inputs, _run
    bwt = load_gz_json("bwt_cluster0.json.gz")
    primers, cluster, unmatched = _inputs(bwt, tmp_path)
    fl = bwt["flags"]
    got = _run(lib, primers, cluster, tmp_path / "cluster.out", fl, gaps=True)
    assert got == bwt["rows"] and len(got) == 485 and sum(len(v) for v in got.values()) == 485
    assert _run(lib, primers, unmatched, tmp_path / "un.out", fl, gaps=True) == {}


def test_bowtie2_fixture_is_unchanged_with_gaps(oracle_lib, tmp_path, capsys):
    """The reference author's bowtie2 run (tests/test_validate_bwt.py: `-l 18 -t 1 -s 50,2000`) with gaps=True: still exactly the 485
    recorded rows on the cluster and no product on the 673 unmatched records.  What this shows is CONSISTENCY with the real mapper —
    admitting the gaps its scoring admits (g <= 2 at the ceiling 11 of an 18-base term) contradicts none of its 1158 recorded
    decisions.  It is not evidence for gaps: the ungapped rule reproduces the same decisions, so the run does not tell the two apart."""
    assert not oracle_lib.gapscan                                   # the host form of the rule is what runs here
    check_bowtie2_fixture_with_gaps(oracle_lib, tmp_path)
    capsys.readouterr()


def test_gaps_switch_changes_only_gapped_sites(oracle_lib, tmp_path, capsys):
    """off_targets(gaps=...) end to end on a planted database: a product whose forward site exists only with a deletion."""
    F, R = make_read(18, seed=3), make_read(18, seed=4)
    rng = np.random.default_rng(77)
    seq = _bases(rng, 300) + site_text(F, "D", 1, 9) + _bases(rng, 150) + rc(R) + _bases(rng, 200)
    (tmp_path / "p.fa").write_text(f">F\n{F}\n>R\n{R}\n")
    (tmp_path / "db.fa").write_text(f">s1\n{seq}\n")
    rows = {}
    for gaps in (False, True):
        out = tmp_path / f"out{int(gaps)}"
        off_targets(str(tmp_path / "p.fa"), 18, str(tmp_path / "db.fa"), "100,1500", 1, str(out), 4, library=oracle_lib, gaps=gaps).run()
        rows[gaps] = out.read_text().splitlines()[1:]
    assert rows[False] == [] and rows[True] == ["s1\t300\t469\tF\tR\t170"]
    capsys.readouterr()
