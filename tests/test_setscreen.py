"""get_Maxprimerset -r on the CPU: the greedy logic around the off-target test, with the pair counts injected
(OffTargetExaminer(table=...)) and the dimer test on the CPU checker library, as in the other set-cover tests.  The counts come
from the model of the rule (tests/setscreen_ref.py) or are written by hand where a case needs one particular number.  The device
side of the same rule is tests/test_setscreen_gpu.py."""
import contextlib
import io
import os
import types

import pytest

import setscreen_cases as cases
import setscreen_ref as ref
from conftest import GOLDEN
from multiprime_amd import maxset
from multiprime_amd.setscreen import OffTargetExaminer, RefusedPrimer, reads_of

FIX = os.path.join(GOLDEN, "setscreen")
FILES = ["final.xls", "final.xls.offtarget.tsv", "final.xls.offtarget.set.tsv", "fina.next.xls", "sort.candidates.txt"]


@pytest.fixture(scope="module")
def golden():
    rows, clusters = cases.golden_case()
    table = ref.pair_table(ref.sites(rows, cases.all_primers(clusters), cases.DIST, 1), 150, 2000)
    assert table, "the model finds no product on the planted background"
    return rows, clusters, table


def run_cover(lib, tmp_path, clusters, table, method="T", sub="run", **kw):
    """the files of one run with injected counts: {name: text or None}, the log rows, the exit status"""
    d = tmp_path / sub
    d.mkdir()
    inp, out = d / "candidates.txt", d / "final.xls"
    inp.write_text(cases.candidate_text(clusters))
    opts = types.SimpleNamespace(input=str(inp), step=5, method=method, out=str(out), device=0, max_offtarget=kw.get("max_offtarget", 0),
                                 cross_only=kw.get("cross_only", False), lookahead=kw.get("lookahead", 4))
    rc = 0
    with contextlib.redirect_stdout(io.StringIO()):
        try:
            maxset.run(opts, library=lib, offtarget=OffTargetExaminer(table=table))
        except SystemExit as e:
            rc = e.code
    files = {n: ((d / n).read_text() if (d / n).exists() else None) for n in FILES}
    log = [line.split("\t") for line in (files["final.xls.offtarget.tsv"] or "").splitlines()[1:]]
    return files, log, rc


def decisions(log):
    return [(r[0], r[1], int(r[4]), int(r[5]), r[6]) for r in log]


def test_recorded_fixture_pins_the_model(oracle_lib, golden, tmp_path):
    rows, clusters, table = golden
    assert open(os.path.join(FIX, "background.fa")).read() == cases.fasta_text(rows)
    assert open(os.path.join(FIX, "candidates.txt")).read() == cases.candidate_text(clusters)
    files, log, rc = run_cover(oracle_lib, tmp_path, clusters, table)
    kinds = {r[6] for r in log}
    assert rc == 0 and kinds == {"selected", "rejected"}
    for name in FILES[:4]:
        assert files[name] == open(os.path.join(FIX, name)).read(), name


def test_own_cross_and_the_exhausted_cluster(oracle_lib, golden, tmp_path):
    _, clusters, table = golden
    files, log, _ = run_cover(oracle_lib, tmp_path, clusters, table)
    d = decisions(log)
    assert ("c3", "1", 2, 0, "rejected") in d                      # by its own products
    assert ("c2", "1", 1, 0, "rejected") in d
    # c1's first pair is clean on its own: it goes because c0's pair entered S before it
    assert d.index(("c0", "1", 0, 0, "selected")) < d.index(("c1", "1", 0, 1, "rejected"))
    assert ("c1", "6", 0, 0, "selected") in d and ("c2", "6", 0, 0, "selected") in d
    # maximal mode: the exhausted cluster is handled as one whose pairs all dimerise
    assert files["fina.next.xls"].split("\t")[0] == "c3" and "\nc3\t\t\t\t\t\t\n" in files["final.xls"]
    # without c0 in front nothing is in S when c1 is walked: the same pair passes
    _, log2, _ = run_cover(oracle_lib, tmp_path, [c for c in clusters if c[0] != "c0"], table, sub="no_c0")
    assert ("c1", "1", 0, 0, "selected") in decisions(log2)


def test_cross_only_and_max_offtarget(oracle_lib, golden, tmp_path):
    _, clusters, table = golden
    base = decisions(run_cover(oracle_lib, tmp_path, clusters, table, sub="a")[1])
    assert ("c3", "1", 2, 0, "rejected") in base and ("c1", "1", 0, 1, "rejected") in base
    cross_only = decisions(run_cover(oracle_lib, tmp_path, clusters, table, sub="b", cross_only=True)[1])
    assert ("c3", "1", 2, 0, "selected") in cross_only              # an own product no longer counts
    assert ("c1", "1", 0, 1, "rejected") in cross_only              # a cross product still does
    files, log, _ = run_cover(oracle_lib, tmp_path, clusters, table, sub="c", max_offtarget=1)
    one = decisions(log)
    assert ("c1", "1", 0, 1, "selected") in one and ("c2", "1", 1, 0, "selected") in one and ("c3", "1", 2, 0, "rejected") in one
    # the set file lists the final set's ordered pairs with a product, sorted by the two strings
    lines = [x.split("\t") for x in files["final.xls.offtarget.set.tsv"].splitlines()]
    assert lines[0] == ["Forward_primer", "Reverse_primer", "Products"] and len(lines) == 3
    assert lines[1:] == sorted(lines[1:]) and all(table[(a, b)] == int(n) for a, b, n in lines[1:])


def test_equal_strings_and_a_reused_primer(oracle_lib, golden, tmp_path):
    _, clusters, _ = golden
    by = dict(clusters)
    f0, r0 = by["c0"][0]
    r2b = by["c2"][1][1]
    # F == R: N has one element, its one self-product counts once
    files, log, _ = run_cover(oracle_lib, tmp_path, [("same", [(r0, r0)])], {(r0, r0): 1}, sub="same", max_offtarget=1)
    assert decisions(log) == [("same", "1", 1, 0, "selected")]
    # a primer already in S comes back in a later pair: it belongs to N, so its products with the new partner are `own`, not `cross`
    table = {(r2b, f0): 1, (f0, r0): 0}
    _, log, _ = run_cover(oracle_lib, tmp_path, [("c0", [(f0, r0)]), ("c2", [(f0, r2b)])], table, sub="reuse", max_offtarget=5)
    assert decisions(log) == [("c0", "1", 0, 0, "selected"), ("c2", "1", 1, 0, "selected")]


def test_maximum_mode_backtracks_and_restores_the_set(oracle_lib, golden, tmp_path):
    _, clusters, _ = golden
    by = dict(clusters)
    xa, xb = by["c1"]
    ya, yb = by["c2"][0], (by["c3"][0][0], by["c2"][1][1])
    za = by["c0"][0]
    filler = [by["c3"][0], by["c2"][0]]
    # X.a enters S; both pairs of Y and Z's first pair amplify with X.a's forward primer only
    table = {(xa[0], ya[1]): 1, (xa[0], yb[1]): 1, (xa[0], za[1]): 3}
    cl = [("X", [xa, xb]), ("Y", [ya, yb]), ("Z", [za] + filler)]
    files, log, rc = run_cover(oracle_lib, tmp_path, cl, table, method="F")
    assert rc == 0
    assert decisions(log) == [("X", "1", 0, 0, "selected"), ("Y", "1", 0, 1, "rejected"), ("Y", "6", 0, 1, "rejected"),
                              ("X", "6", 0, 0, "selected"), ("Z", "1", 0, 0, "selected")]      # Z sees S without X.a again
    picked = [line.split("\t")[:2] for line in files["final.xls"].splitlines()[1:]]
    assert picked == [["X", "6"], ["Z", "1"]]
    assert files["final.xls.offtarget.set.tsv"] == "Forward_primer\tReverse_primer\tProducts\n"


def test_files_do_not_depend_on_the_lookahead(oracle_lib, golden, tmp_path):
    _, clusters, table = golden
    a = run_cover(oracle_lib, tmp_path, clusters, table, sub="k1", lookahead=1)
    b = run_cover(oracle_lib, tmp_path, clusters, table, sub="k1000", lookahead=1000)
    assert a[0] == b[0] and "rejected" in a[0]["final.xls.offtarget.tsv"] and "selected" in a[0]["final.xls.offtarget.tsv"]


def test_reads_follow_the_term_rule():
    assert reads_of("ACGTACGTACGTAR", 12) == ["GTACGTACGTAA", "GTACGTACGTAG"]
    assert reads_of("ACGTAC", 12) == ["ACGTAC"] and reads_of("ACGTACGTACGTACGT", 0) == ["ACGTACGTACGTACGT"]
    for bad in ("ACG", "ACGTacgt", "ACGTXCGT", "A" * 65):
        with pytest.raises(RefusedPrimer, match=bad):
            reads_of(bad, 0)


def cli(argv, capsys):
    with pytest.raises(SystemExit) as e:
        maxset.main(argv)
    return e.value.code, capsys.readouterr().err


def test_refusals_exit_before_anything_is_written(golden, tmp_path, capsys, monkeypatch):
    monkeypatch.setenv("MP_KEEP_PIN_THRESHOLD", "1")          # main() leaves the process's runtime settings alone
    rows, clusters, _ = golden
    inp, bg, out = tmp_path / "candidates.txt", tmp_path / "bg.fa", tmp_path / "final.xls"
    inp.write_text(cases.candidate_text(clusters))
    bg.write_text(cases.fasta_text(rows))
    base = ["-i", str(inp), "-o", str(out)]

    def untouched():
        return sorted(p.name for p in tmp_path.iterdir()) == ["bg.fa", "candidates.txt", "empty.fa", "headers.fa"]

    (tmp_path / "empty.fa").write_text("")
    (tmp_path / "headers.fa").write_text(">a\n>b\n")
    for ref_file in ("missing.fa", "empty.fa", "headers.fa"):
        code, err = cli(base + ["-r", str(tmp_path / ref_file)], capsys)
        assert code == 1 and ref_file in err and untouched()
    for bad in ("ACG", "ACGTNNacgtACGTACGTAC", "ACGTACGTAC*TACGTACGT"):
        inp.write_text(cases.candidate_text(clusters + [("bad", [(bad, clusters[0][1][0][1])])]))
        code, err = cli(base + ["-r", str(bg)], capsys)
        assert code == 1 and repr(bad) in err and untouched()
    inp.write_text(cases.candidate_text(clusters))
    for extra in (["-p", "abc"], ["-p", "2000,150"], ["-p", "150"], ["-d", "-1"], ["--seedmms", "4"], ["--seedmms", "-1"],
                  ["--max-offtarget", "-1"], ["--lookahead", "0"]):
        code, _ = cli(base + ["-r", str(bg)] + extra, capsys)
        assert code == 2 and untouched(), extra
