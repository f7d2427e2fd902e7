"""The host side of the DegePrime drop-ins and the yardstick itself, without a GPU: scripts/TrimAlignment.py against the bytes the Perl
script wrote, tests/dege_ref.py against the tables DegePrime.pl wrote (the window numbers) and against an exhaustive search (the
merging), the reduction of -d, the refusals, and the quality condition of the rule on dege_wide (tests/golden/make_golden_dege.py)."""
import os
import subprocess
import sys

import pytest

import dege_cases as cases
import dege_ref as ref
from conftest import REPO, load_gz_json
from multiprime_amd import degeprime

TRIM = os.path.join(REPO, "scripts", "TrimAlignment.py")
RUN = os.path.join(REPO, "scripts", "run_dege.py")


@pytest.fixture(scope="module")
def golden():
    return load_gz_json("dege.json.gz")


def rows_of(text):
    return [s for _, s in ref.read_fasta(text)]


def run(script, args, cwd):
    return subprocess.run([sys.executable, script] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("name", sorted(cases.TRIMS))
def test_trim_reproduces_the_recorded_bytes(name, golden, tmp_path):
    g = golden["small"]
    assert g["input"] == cases.small_fasta() and g["trims"][name]["flags"] == cases.TRIMS[name]
    (tmp_path / "in.fa").write_text(g["input"])
    degeprime.trim_main(["-i", str(tmp_path / "in.fa"), "-o", str(tmp_path / "out.fa")] + cases.TRIMS[name])
    assert (tmp_path / "out.fa").read_bytes() == g["trims"][name]["text"].encode()


def test_trim_marks_what_the_cases_are_about(golden):
    """The recorded outputs do hold what the issue asks them to cover: lower-case marks, U -> T, '.', and no mark after the last kept
    column."""
    t = golden["small"]["trims"]
    assert any(ch.islower() for ch in t["min05"]["text"].replace(">s", "").replace(">ref", ""))
    assert "U" not in t["default"]["text"].upper().replace(">", "") and "." in t["default"]["text"]
    assert all(not row[-1].islower() for row in rows_of(t["ref"]["text"]))
    assert len({len(r) for name in t for r in rows_of(t[name]["text"])}) > 2


def test_trim_command_line_on_the_slices(golden, tmp_path):
    """The script as a command, on the 150 x 320 slice (default flags: nothing but upper-casing happens to the columns it keeps)."""
    (tmp_path / "in.fa").write_text(golden["dege_sub"]["input"])
    r = run(TRIM, ["-i", "in.fa", "-o", "out.fa"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.fa").read_bytes() == golden["dege_sub"]["trim"].encode()


def first_columns(table):
    return [line.split("\t") for line in table.splitlines()[1:]]


@pytest.fixture(scope="module")
def wide_windows(golden):
    g = golden["dege_wide"]
    return ref.windows(rows_of(g["trim"]), g["flags"]["l"], g["flags"]["skip"])


def check_window_numbers(table, wins, depth=1):
    rec = first_columns(table)
    assert table.splitlines()[0] == ref.HEADER
    printed = [(pos, w) for pos, w in enumerate(wins) if w[1] >= depth]
    assert [int(r[0]) for r in rec] == [pos for pos, _ in printed]
    for r, (pos, (n, z, ent, uniq)) in zip(rec, printed):
        assert (int(r[1]), int(r[2])) == (n, len(uniq)), pos
        assert abs(float(r[3]) - ent) <= 1e-9, (pos, r[3], ent)
        assert sum(c for _, c in uniq) == z


def test_ref_window_numbers_equal_perl_on_dege_sub(golden):
    g = golden["dege_sub"]
    assert g["flags"] == cases.SUB_FLAGS
    check_window_numbers(g["table"], ref.windows(rows_of(g["trim"]), g["flags"]["l"]))


def test_ref_window_numbers_equal_perl_on_dege_wide(golden, wide_windows):
    assert golden["dege_wide"]["flags"] == cases.WIDE_FLAGS
    check_window_numbers(golden["dege_wide"]["table"], wide_windows)


def test_ref_window_numbers_equal_perl_on_a_lower_case_trim(golden):
    t = golden["small"]["table"]
    of, flags = cases.SMALL_TABLE
    assert (t["of"], t["flags"]) == (of, flags)
    opt = dict(zip(flags[::2], flags[1::2]))
    rows = rows_of(golden["small"]["trims"][of]["text"])
    assert any(ch.islower() for r in rows for ch in r)
    check_window_numbers(t["text"], ref.windows(rows, int(opt["-l"]), int(opt["-skip"])))
    assert len(first_columns(t["text"])) >= 10


def test_quality_of_the_rule_on_dege_wide(golden, wide_windows):
    """Summed NumberMatching at seed 0 against the three Perl runs: not below the smallest by more than their own spread."""
    g = golden["dege_wide"]
    totals = [sum(run) for run in g["matching"]]
    assert len(totals) == 3
    f = g["flags"]
    d = ref.valid_degeneracy(f["d"])
    total = 0
    for pos, (n, z, ent, uniq) in enumerate(wide_windows):
        if z >= 1:
            its, best = ref.merge(uniq, f["l"], d, 100, 0, pos)
            total += its[best][1]
    print("dege_wide: Perl", totals, "rule", total)
    assert total >= min(totals) - (max(totals) - min(totals)), (total, totals)


@pytest.mark.parametrize("d, want", [(5, 4), (7, 6), (10, 9), (11, 9), (1, 1), (12, 12), (2 ** 20 * 3 ** 5 + 1, 2 ** 20 * 3 ** 5)])
def test_degeneracy_reduction(d, want):
    assert ref.valid_degeneracy(d) == want and degeprime.valid_degeneracy(d) == want


def test_table_formatting():
    assert degeprime.fmt(0.0) == "0" and degeprime.fmt(-0.0) == "0" and degeprime.fmt(1 / 3) == "0.333333333333333"
    assert degeprime.fmt(2.5849625007211565) == "2.58496250072116" and ref.fmt(150 / 150) == "1"
    assert [ref.IUPAC[ref.SET_OF[m]] for m in range(1, 16)] == list(degeprime.SET_LETTER[1:])


REFUSALS = [
    (TRIM, "dots", [], "nothing but '.'"),
    (TRIM, "ragged", [], "different lengths"),
    (TRIM, "small", ["-ref", "nobody"], "was not found"),
    (TRIM, "small", ["-min", "0.5", "-ref", "ref1"], "both minimum occupancy and reference"),
    (RUN, "small", ["-taxfile", "tax.txt"], "not served"),
    (RUN, "small", ["-taxlevel", "3"], "not served"),
    (RUN, "ragged", [], "same length"),
    (RUN, "small", ["-l", "33"], "2..32"),
]


@pytest.mark.parametrize("script, which, flags, sentence", REFUSALS,
                         ids=["%s-%s-%s" % (os.path.basename(r[0]), r[1], "_".join(r[2]) or "default") for r in REFUSALS])
def test_refusals_exit_with_status_2_and_a_sentence(script, which, flags, sentence, tmp_path):
    text = {"small": cases.small_fasta(), "ragged": ">a\nACGT\n>b\nACG\n", "dots": ">a\nAC.T\n>b\nAG.T\n"}[which]
    (tmp_path / "in.fa").write_text(text)
    r = run(script, ["-i", "in.fa", "-o", "out.txt"] + flags, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert sentence in r.stderr, r.stderr
    assert not (tmp_path / "out.txt").exists() and not (tmp_path / "out.txt.tmp").exists()


def synthetic_windows():
    out = []
    for seed in range(6):
        rows = cases.random_rows(40 + 7 * seed, 5, 100 + seed, n_variants=2 + seed)
        n, z, ent, uniq = ref.windows(rows, 5, 0)[0]
        out.append((seed, z, uniq))
    out.append((99, 30, [(ref.word_of(m), 1) for m in cases.distinct_rows(30, 5, 3)]))
    return out


@pytest.mark.parametrize("seed, z, uniq", synthetic_windows())
def test_merging_against_the_exhaustive_optimum(seed, z, uniq):
    """l = 5, d = 4: no iteration beats the best oligomer there is, and what it reports is what its oligomer matches."""
    best_possible = ref.optimum(uniq, 5, 4)
    its, best = ref.merge(uniq, 5, 4, 100, seed, 0)
    for deg, match, n_draws, sets in its:
        primer = "".join(ref.IUPAC[s] for s in sets)
        assert match == ref.recount(primer, uniq, 5) <= best_possible
        prod = 1
        for s in sets:
            prod *= len(s)
        assert deg == prod <= 4 and 1 <= n_draws <= min(100, len(uniq))
    assert its[best][1] == max(x[1] for x in its) and all(x[1] < its[best][1] for x in its[:best])
    assert its[best][1] >= max(c for _, c in uniq)


def test_draws_are_integers_with_the_stated_distribution():
    """draw() stays below R, differs between seeds, and over many t lands on a mer about in proportion to its count."""
    assert all(0 <= ref.draw(s, 3, 7, t, 10) < 10 for s in (0, 1) for t in range(100))
    assert [ref.draw(0, 0, 0, t, 1 << 30) for t in range(8)] != [ref.draw(1, 0, 0, t, 1 << 30) for t in range(8)]
    hits = sum(ref.draw(0, 5, it, 0, 100) < 25 for it in range(4000))
    assert 850 <= hits <= 1150           # binomial(4000, 0.25): sd 27
    assert ref.mix(0) == 0 and ref.mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF           # splitmix64's first output for the state 0
