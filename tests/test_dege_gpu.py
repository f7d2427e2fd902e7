"""DegePrime on the device (csrc/dege.hip behind mp_dege_load / mp_dege_windows / mp_dege_merge) against the yardstick of
tests/dege_ref.py on the cases of tests/dege_cases.py: every integer and every set equal, the entropy to 1e-9; then scripts/run_dege.py on
the recorded slices, the quality condition against the Perl runs, and the three scripts of the workflow in a row."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dege_cases as cases
import dege_ref as ref
from conftest import REPO, load_gz_json
from multiprime_amd._abi import DEGE_LDS_LIMIT, DEGE_REC, MprimeError
from multiprime_amd.degeprime import DegePrime, read_trimmed

TRIM = os.path.join(REPO, "scripts", "TrimAlignment.py")
RUN = os.path.join(REPO, "scripts", "run_dege.py")
PAIR = os.path.join(REPO, "scripts", "get_degePrimer.py")


def matrix(rows):
    return np.frombuffer("".join(rows).encode(), np.uint8).reshape(len(rows), len(rows[0]))


def sets_of(rec, l):
    return [ref.SET_OF[int(m)] for m in rec[3:3 + l]]


def check_windows(ctx, rows, l, skip, depth=1):
    """Load, run the window stage and compare every window with the yardstick; returns (nums, yardstick windows)."""
    ctx.dege_load(matrix(rows))
    nums, ent = ctx.dege_windows(l, skip, depth)
    want = ref.windows(rows, l, skip)
    assert len(nums) == len(want) == len(rows[0]) - l + 1
    for pos, (n, z, e, uniq) in enumerate(want):
        assert nums[pos].tolist() == [n, z, len(uniq), int(z >= depth)], (pos, nums[pos], n, z, len(uniq))
        assert abs(ent[pos] - e) <= 1e-9, (pos, ent[pos], e)
        words, counts = ctx.dege_unique(pos)
        assert words.tolist() == [w for w, _ in uniq] and counts.tolist() == [c for _, c in uniq], pos
    return nums, want


def check_merge(ctx, want, l, max_deg, iters, seed, depth=1, positions=None):
    """Run the merging and compare the winner of every printed window and every iteration of `positions` (default: all printed)."""
    best = ctx.dege_merge(max_deg, iters, seed)
    assert best.shape == (len(want), DEGE_REC)
    for pos, (n, z, e, uniq) in enumerate(want):
        if z < depth:
            assert (best[pos] == -1).all(), pos
            continue
        if positions is not None and pos not in positions:
            continue
        its, k = ref.merge(uniq, l, max_deg, iters, seed, pos)
        got = ctx.dege_iterations(pos)
        assert got.shape == (iters, DEGE_REC)
        for it, (deg, match, n_draws, sets) in enumerate(its):
            assert got[it, :3].tolist() == [deg, match, n_draws] and sets_of(got[it], l) == sets, (pos, it, got[it], its[it])
            assert (got[it, 3 + l:] == 0).all()
        deg, match, _, sets = its[k]
        assert best[pos, :3].tolist() == [match, deg, k] and sets_of(best[pos], l) == sets, (pos, best[pos], its[k], k)
    return best


@pytest.fixture
def ctx(hip_lib):
    assert hip_lib.backend == "hip" and hip_lib.dege
    c = hip_lib.context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return load_gz_json("dege.json.gz")


# ---- the window stage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", cases.WINDOW_ROWS)
def test_windows_rows(n_rows, ctx):
    rows = cases.random_rows(n_rows, 40, 10 + n_rows, p_gap=0.02, p_lower=0.03, p_dot=0.3, p_iupac=0.01, lead=8)
    check_windows(ctx, rows, 12, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", (0, 1))
def test_windows_width(extra, ctx):
    rows = cases.random_rows(50, 18 + extra, 5, p_lower=0.02)
    nums, _ = check_windows(ctx, rows, 18, 0)
    assert len(nums) == 1 + extra


@pytest.mark.gpu
@pytest.mark.parametrize("l", cases.WINDOW_L)
def test_windows_primer_lengths(l, ctx):
    rows = cases.random_rows(90, l + 5, 20 + l, p_gap=0.01, p_lower=0.02, p_iupac=0.01, n_variants=3)
    rows += ["T" * (l + 5), "A" * (l + 5), "T" * (l + 4) + "t"]           # the largest and the smallest word, and a lower-case last byte
    nums, want = check_windows(ctx, rows, l, 0)
    assert any(u[-1][0] == (1 << (2 * l)) - 1 and u[-1][1] >= 2 and u[0][0] == 0 for _, _, _, u in want)
    check_merge(ctx, want, l, 6, 8, 3, positions={0, 5})


@pytest.mark.gpu
def test_windows_refuse_other_lengths_and_bytes(ctx):
    rows = cases.random_rows(4, 40, 1)
    ctx.dege_load(matrix(rows))
    for l in (0, 1, 33):
        with pytest.raises(MprimeError, match=r"primer length"):
            ctx.dege_windows(l, 0, 1)
    with pytest.raises(MprimeError, match=r"depth"):
        ctx.dege_windows(18, 0, 0)
    assert ctx.dege_windows(32, 0, 1)[0].shape == (9, 4)
    bad = [r for r in rows]
    bad[2] = bad[2][:17] + "X" + bad[2][18:]
    bad[3] = bad[3][:5] + "*" + bad[3][6:]
    with pytest.raises(MprimeError, match=r"row 2, column 17: byte 0x58"):
        ctx.dege_load(matrix(bad))
    with pytest.raises(MprimeError, match=r"mp_dege_load first"):
        ctx.dege_windows(18, 0, 1)


@pytest.mark.gpu
def test_windows_span_bounds_case_and_gap_marks(ctx):
    l, skip = 6, 3
    rows, pos = cases.span_rows(l, skip)
    nums, want = check_windows(ctx, rows, l, skip)
    # at pos: rows 0 and 3 (bounds hit / to spare), the full row and its four marked copies span; rows 1 and 2 miss by one
    assert nums[pos].tolist() == [7, 4, 1, 1]
    assert nums[pos - 1, 0] == 6 and nums[pos + 1, 0] == 6                 # each neighbour loses the row that hit one bound exactly
    assert nums[0].tolist() == [0, 0, 0, 0] and nums[-1].tolist() == [0, 0, 0, 0]         # nobody spans
    # entropy at pos: one mer four times and three different marked ones
    e = -(4 / 7) * np.log2(4 / 7) - 3 * (1 / 7) * np.log2(1 / 7)
    assert abs(ctx.dege_windows(l, skip, 1)[1][pos] - e) <= 1e-9
    check_merge(ctx, want, l, 4, 5, 0)
    # a window that rows span and none is gap-free in
    rows = ["ACGTNACGTACGT", "ACGTRACGTACGT", "ACGTnACGTACGA"]
    nums, want = check_windows(ctx, rows, 5, 0)
    assert nums[2].tolist() == [3, 0, 0, 0] and nums[5].tolist() == [3, 3, 1, 1] and nums[8].tolist() == [3, 3, 2, 1]
    check_merge(ctx, want, 5, 2, 3, 0)
    nums, want = check_windows(ctx, rows, 5, 0, depth=3)
    assert nums[:, 3].tolist() == [0] * 5 + [1] * 4


@pytest.mark.gpu
@pytest.mark.parametrize("u", cases.UNIQUE_SIZES)
def test_windows_unique_counts_around_every_path_change(u, ctx):
    """One window of U distinct gap-free mers; the first rows repeated, so that counts differ."""
    rows = cases.distinct_rows(u, 8, seed=u, repeats=(3, 1)[:u])
    check_windows(ctx, rows, 8, 0)
    assert ctx.dege_stats()[1]["global_windows"] == int(u > DEGE_LDS_LIMIT)
    assert ctx.dege_stats()[1]["unique"] == u


@pytest.mark.gpu
def test_windows_unique_equals_rows_and_marked_mers_count_towards_the_table(ctx):
    rows = cases.distinct_rows(65, 8, seed=7)
    nums, _ = check_windows(ctx, rows, 8, 0)
    assert nums[0].tolist() == [65, 65, 65, 1]
    # U below the limit of the LDS table, the distinct mers of all spanning rows above it: the global table
    rows = cases.distinct_rows(DEGE_LDS_LIMIT - 2, 8, seed=9)
    rows += [r[:3] + "n" + r[4:] for r in rows[:5]]
    nums, _ = check_windows(ctx, rows, 8, 0)
    assert nums[0].tolist() == [DEGE_LDS_LIMIT + 3, DEGE_LDS_LIMIT - 2, DEGE_LDS_LIMIT - 2, 1]
    assert ctx.dege_stats()[1]["global_windows"] == 1


@pytest.mark.gpu
def test_windows_mixed_paths_in_one_alignment(ctx):
    """Windows of one alignment on different paths: every row differs in the first window, the later ones hold fewer distinct mers."""
    rows = [r + "AC" for r in cases.distinct_rows(DEGE_LDS_LIMIT + 9, 7, seed=4)]
    nums, want = check_windows(ctx, rows, 7, 0)
    over = [len(u) > DEGE_LDS_LIMIT for _, _, _, u in want]
    assert over[0] and not over[2] and ctx.dege_stats()[1]["global_windows"] == sum(over)
    check_merge(ctx, want, 7, 4, 4, 0)


# ---- the merging ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("u", cases.MERGE_SIZES)
def test_merge_unique_sizes_all_counts_one(u, ctx):
    rows = cases.distinct_rows(u, 8, seed=100 + u)
    nums, want = check_windows(ctx, rows, 8, 0)
    assert nums[0].tolist() == [u, u, u, 1]
    check_merge(ctx, want, 8, 12, 100 if u <= 101 else 12, 0)


@pytest.mark.gpu
def test_merge_one_mer_holds_almost_all_rows(ctx):
    """The drawn index is corrected by what was removed: the heavy mer goes early, every later draw lands beyond it."""
    for heavy in (0, 50, 100):
        rows = cases.distinct_rows(101, 8, seed=11)
        order = sorted(rows)
        rows += [order[heavy]] * 400
        _, want = check_windows(ctx, rows, 8, 0)
        check_merge(ctx, want, 8, 2 ** 20 * 3 ** 5, 20, heavy)


@pytest.mark.gpu
@pytest.mark.parametrize("d", cases.MERGE_DEGS)
def test_merge_degeneracies(d, ctx):
    rows = cases.random_rows(200, 16, 77, n_variants=6)
    _, want = check_windows(ctx, rows, 12, 0)
    best = check_merge(ctx, want, 12, d, 10, 5)
    assert (best[:, 1] <= d).all() and (best[:, 1] >= 1).all()


@pytest.mark.gpu
def test_merge_product_saturates_at_32_letters(ctx):
    """l = 32 and four letters at every position: the product of the set sizes passes 2^64 on the way."""
    rows = cases.distinct_rows(120, 32, seed=5)
    assert all(len({r[p] for r in rows}) == 4 for p in range(32))
    _, want = check_windows(ctx, rows, 32, 0)
    for d in (4, 2 ** 20 * 3 ** 5, 2 ** 31 - 1):
        check_merge(ctx, want, 32, d, 6, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("iters", cases.MERGE_ITERS)
def test_merge_iteration_counts(iters, ctx):
    rows = cases.random_rows(60, 14, 31, n_variants=5)
    _, want = check_windows(ctx, rows, 10, 0)
    check_merge(ctx, want, 10, 6, iters, 2, positions={0, 4})
    with pytest.raises(MprimeError, match="iterations"):
        ctx.dege_merge(6, 65537, 0)
    with pytest.raises(MprimeError, match="degeneracy"):
        ctx.dege_merge(0, 10, 0)


@pytest.mark.gpu
def test_merge_seeds_and_repeatability(ctx, hip_lib):
    rows = cases.random_rows(150, 30, 8, p_gap=0.01, p_lower=0.01, n_variants=8, lead=3)
    m = matrix(rows)
    out = []
    for seed in (0, 0, 1):
        c = hip_lib.context(0)
        try:
            c.dege_load(m)
            nums, ent = c.dege_windows(12, 2, 1)
            best = c.dege_merge(6, 50, seed)
            pos = int(np.flatnonzero(nums[:, 3])[3])
            out.append((nums.tobytes(), ent.tobytes(), best.tobytes(), c.dege_iterations(pos).tobytes(), c.dege_iterations(pos)[:, 2].sum()))
        finally:
            c.close()
    assert out[0] == out[1]
    assert out[0][:2] == out[2][:2] and out[0][3] != out[2][3]
    its = ref.merge(ref.windows(rows, 12, 2)[pos][3], 12, 6, 50, 1, pos)[0]
    assert sum(x[2] for x in its) == out[2][4]


@pytest.mark.gpu
@pytest.mark.parametrize("d", (4, 12))
def test_merge_matches_every_row_when_the_union_fits(d, ctx):
    """U <= 100 and the union of all mers within max_deg: every iteration ends on the union and matches all Z rows."""
    base = "ACGTTGCAAGGC"
    rows = [base[:3] + a + base[4:8] + b + base[9:] for a in "AC" for b in "GT" for _ in range(3)] + [base[:3] + "A" + base[4:8] + "G" + base[9:]] * 5
    nums, want = check_windows(ctx, rows, 12, 0)
    best = check_merge(ctx, want, 12, d, 30, 0)
    assert nums[0].tolist() == [17, 17, 4, 1] and best[0, :2].tolist() == [17, 4]
    assert (ctx.dege_iterations(0)[:, 1] == 17).all()


# ---- the drop-in ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sub_table(golden):
    g = golden["dege_sub"]
    rows = [s for _, s in ref.read_fasta(g["trim"])]
    return rows, ref.table_text(rows, g["flags"]["l"], ref.valid_degeneracy(g["flags"]["d"]))


@pytest.mark.gpu
def test_run_dege_on_dege_sub(golden, sub_table, tmp_path, hip_lib):
    g = golden["dege_sub"]
    rows, want = sub_table
    (tmp_path / "trim.fa").write_text(g["trim"])
    r = subprocess.run([sys.executable, RUN, "-i", "trim.fa", "-o", "table.txt", "-s", "nowhere", "-l", str(g["flags"]["l"]), "-d", str(g["flags"]["d"])],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = (tmp_path / "table.txt").read_text()
    assert not (tmp_path / "table.txt.tmp").exists()
    assert got == want
    wins = ref.windows(rows, g["flags"]["l"])
    total = 0
    for line in got.splitlines()[1:]:
        f = line.split("\t")
        size = 1
        for ch in f[5]:
            size *= len(ref.IUPAC_SET[ch])
        assert int(f[4]) == size <= g["flags"]["d"], line
        assert int(f[6]) == ref.recount(f[5], wins[int(f[0])][3], g["flags"]["l"]), line
        total += int(f[6])
    perl = sum(int(line.split("\t")[6]) for line in g["table"].splitlines()[1:])
    print("dege_sub: Perl", perl, "drop-in", total)
    assert total >= perl
    # -d 11 is lowered to 9, with Perl's sentence
    r = subprocess.run([sys.executable, RUN, "-i", "trim.fa", "-o", "t11.txt", "-l", "18", "-d", "11", "--iter", "3", "--seed", "4", "--skip", "30",
                        "--depth", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Max degeneracy was not a valid degeneracy and has been changed to 9" in r.stdout, r.stderr
    assert (tmp_path / "t11.txt").read_text() == ref.table_text(rows, 18, 9, skip=30, depth=2, iters=3, seed=4)


@pytest.mark.gpu
def test_quality_of_the_drop_in_on_dege_wide(golden, hip_lib, tmp_path):
    g = golden["dege_wide"]
    totals = [sum(run) for run in g["matching"]]
    (tmp_path / "trim.fa").write_text(g["trim"])
    f = g["flags"]
    job = DegePrime(str(tmp_path / "trim.fa"), str(tmp_path / "table.txt"), f["l"], f["d"], f["skip"], library=hip_lib)
    job.run()
    rec = [line.split("\t") for line in (tmp_path / "table.txt").read_text().splitlines()[1:]]
    assert [r[:3] for r in rec] == [line.split("\t")[:3] for line in g["table"].splitlines()[1:]]
    total = sum(int(r[6]) for r in rec)
    print("dege_wide: Perl", totals, "drop-in", total, job.stats)
    assert total >= min(totals) - (max(totals) - min(totals)), (total, totals)


@pytest.mark.gpu
def test_run_dege_refuses_a_byte_outside_the_alphabet(tmp_path):
    (tmp_path / "trim.fa").write_text(">a\nACGTACGTAC\n>b\nACGTAC!TAC\n")
    r = subprocess.run([sys.executable, RUN, "-i", "trim.fa", "-o", "table.txt", "-l", "4", "--skip", "0"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2 and "row 1, column 6" in r.stderr, (r.returncode, r.stderr)
    assert not (tmp_path / "table.txt").exists()


@pytest.mark.gpu
def test_trim_then_dege_then_pairs(golden, tmp_path):
    """Rules 7, 8 and 9 of the workflow in a row: TrimAlignment.py -> run_dege.py -> get_degePrimer.py writes its output."""
    (tmp_path / "cluster.msa").write_text(golden["dege_sub"]["input"])
    (tmp_path / "cluster.fa").write_text(golden["dege_sub"]["input"].replace("-", ""))
    for cmd in ([TRIM, "-i", "cluster.msa", "-o", "cluster.trim.msa", "-min", "0.9"],
                [RUN, "-i", "cluster.trim.msa", "-o", "cluster.dege.out", "-l", "18", "-d", "12"],
                [PAIR, "-i", "cluster.dege.out", "-r", "cluster.fa", "-o", "cluster.candidate.txt", "-f", "0.3", "-s", "100,300", "-g", "0.2,0.7", "-p", "1"]):
        r = subprocess.run([sys.executable] + cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (cmd, r.stderr[-2000:])
    rows = read_trimmed(str(tmp_path / "cluster.trim.msa"))
    assert rows.shape[0] == 150 and rows.shape[1] < 320
    table = (tmp_path / "cluster.dege.out").read_text().splitlines()
    assert table[0] == ref.HEADER and len(table) > 100
    assert (tmp_path / "cluster.candidate.txt").stat().st_size > 0
