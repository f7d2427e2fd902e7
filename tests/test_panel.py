"""The panel update without a GPU: tests/panel_ref.py against what the unmodified reference wrote (tests/golden/panel/, recorded by
make_golden_panel.py), the host path of multiprime_amd/panel.py against panel_ref.py in exact order, the tables handed to the device
against direct evaluation, and the command line."""
import os
import shutil

import numpy as np
import pytest

import panel_ref as R
from conftest import GOLDEN, REPO
from multiprime_amd import panel

PANEL = os.path.join(GOLDEN, "panel")


def lines_of(path):
    with open(path) as f:
        text = f.read().split("\n")
    assert text[-1] == ""
    return text[0], text[1:-1]


def case_copy(tmp_path, case):
    for name in os.listdir(os.path.join(PANEL, case)):
        if not name.startswith("out."):
            shutil.copy(os.path.join(PANEL, case, name), tmp_path)
    return str(tmp_path / "core.fa"), str(tmp_path / "new.fa")


# ---- panel_ref.py against the reference's own files ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["plain", "degenerate"])
def test_ref_dimer_lines_are_the_references(case):
    head, want = lines_of(os.path.join(PANEL, case, "out.dimer"))
    assert head == "\t".join(R.DIMER_HEADER)
    got = R.dimer_lines(os.path.join(PANEL, case, "core.fa"), os.path.join(PANEL, case, "new.fa"))
    assert sorted(got) == sorted(want) and len(want) >= 5
    head, want_num = lines_of(os.path.join(PANEL, case, "out.dimer.dimer_num"))
    assert head == R.NUM_HEADER
    assert set(R.count_lines(got, 0, 7)) == set(want_num) and len(want_num) == len(set(want_num))


def test_plain_case_holds_what_it_is_for():
    _, want = lines_of(os.path.join(PANEL, "plain", "out.dimer"))
    cols = [line.split("\t") for line in want]
    assert any(want.count(line) == 2 for line in want)                                    # the common sequence runs twice
    assert any(int(c[9]) >= 21 and float(c[10]) <= 3 and float(c[3]) < -5 for c in cols)  # deltaG alone, far from the 3' end
    assert any(int(c[9]) > 0 and float(c[10]) > 3 for c in cols) and any(c[0] == ">n1_again" for c in cols)
    assert any("|" in c[0] for c in cols) and any(int(c[4]) == 4 for c in cols)


def test_ref_offtarget_lines_are_the_references():
    head, want = lines_of(os.path.join(PANEL, "sam", "out.offtargets"))
    assert head == "\t".join(R.OFFTARGET_HEADER)
    got = R.offtarget_lines(os.path.join(PANEL, "sam", "core.fa"), os.path.join(PANEL, "sam", "new.fa"), 100, 1500)
    assert sorted(got) == sorted(want) and len(want) >= 15
    # per gene: the same genes and the same lines in the same order within each gene (a gene's lines of the three joins, in join order)
    def by_gene(lines):
        out = {}
        for line in lines:
            out.setdefault(line.split("\t")[0], []).append(line)
        return out
    assert by_gene(got) == by_gene(want)
    head, want_num = lines_of(os.path.join(PANEL, "sam", "out.offtargets.num"))
    assert head == R.NUM_HEADER
    assert set(R.count_lines(got, 3, 4)) == set(want_num)


def test_sam_case_holds_what_it_is_for():
    _, want = lines_of(os.path.join(PANEL, "sam", "out.offtargets"))
    cols = [line.split("\t") for line in want]
    genes = {c[0] for c in cols}
    assert genes == {"g1", "g2", "g3"}                                   # g4, g5: the early outs; g6: one strand only
    assert not any(c[5] in ("100", "1500") for c in cols) and any(c[5] == "101" for c in cols) and any(c[5] == "1499" for c in cols)
    assert any(c[0] == "g1" and c[1] == "1000" and c[3] == "cA_0|>cB_0" for c in cols)       # the last of three lines wins
    assert any(c[0] == "g1" and c[1] == "1000" and c[3] == "nA_0" for c in cols)             # and the new file keeps the start too
    assert not any(c[0] == "g3" and c[1] == "5000" for c in cols)                            # the dead start ended the gene
    assert not any(c[0] == "g2" and c[1] in ("100", "110", "130") for c in cols)             # MD:Z endings 4, 3A4, 9A0


def test_sam_rule_is_not_validates_reader():
    """validate.sites_of_sam(path, 5) applies the same MD:Z test but names a site by its primer (the read's index is cut off); PU keeps
    the read name — the positions agree, the names do not."""
    from multiprime_amd.validate import sites_of_sam
    p = os.path.join(PANEL, "sam", "core.for.sam")
    mine, theirs = panel.sam_sites(p), sites_of_sam(p, 5)
    assert {g: sorted(dict(v)) for g, v in mine.items()} == {g: sorted(v) for g, v in theirs.items()}
    assert dict(mine["g1"])[1000] == "cA_0|>cB_0" and theirs["g1"][1000] != "cA_0|>cB_0"
    assert {g: dict(v) for g, v in mine.items()} == R.sam_sites(p)


# ---- the host path of panel.py against panel_ref.py, exact order ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["plain", "degenerate"])
def test_host_dimer_files(tmp_path, case):
    core, new = case_copy(tmp_path, case)
    out = str(tmp_path / "o.dimer")
    panel.Dimer(core, new, out, nproc=3, search="host").run()
    head, got = lines_of(out)
    want = R.dimer_lines(core, new)
    assert head == "\t".join(R.DIMER_HEADER) and got == want
    head, got_num = lines_of(out + ".dimer_num")
    assert head == R.NUM_HEADER and got_num == R.count_lines(want, 0, 7)
    assert not any(n.endswith(".primer_set") for n in os.listdir(tmp_path))           # the reference's caches are not written


def test_host_cross_records_equal_the_restatement():
    from panel_cases import degenerate_set, length_set
    for seqs, jobs in (length_set(), degenerate_set()):
        assert panel.host_cross(seqs, jobs) == R.cross_records(seqs, jobs)


def test_host_offtarget_files_from_sam(tmp_path):
    core, new = case_copy(tmp_path, "sam")
    out = str(tmp_path / "o.offtargets")
    panel.off_targets(core, new, 1, 9, "", "100,1500", out, 4, join="host").run()
    head, got = lines_of(out)
    want = R.offtarget_lines(core, new, 100, 1500)
    assert head == "\t".join(R.OFFTARGET_HEADER) and got == want
    head, got_num = lines_of(out + ".num")
    assert head == R.NUM_HEADER and got_num == R.count_lines(want, 3, 4)
    # the reads of get_term (PU:379-408): written when absent, names joined with '|', one record per concrete sequence
    assert open(tmp_path / "core.term.fa").read() == ">cA_0\nAGGACCTGA\n>cB_0\nAGTCCGATG\n"
    assert not any(n.endswith(".gene_position") for n in os.listdir(tmp_path))


def test_term_reads_group_and_expand(tmp_path):
    p = tmp_path / "p.fa"
    p.write_text(">a\nACGTACGTRC\n>b\nTTTTACGTRC\n>c\nGGGGGGACGTAC\n")
    assert panel.term_reads(p, 6) == [(">a|>b_0|>c_0", "ACGTAC"), (">a|>b_1", "ACGTGC")]
    assert [s for _, s in panel.term_reads(p, 0)] == ["ACGTACGTAC", "ACGTACGTGC", "TTTTACGTAC", "TTTTACGTGC", "GGGGGGACGTAC"]


def test_joins_equal_amplicons():
    """PU:427-454 against validate.amplicons() on random site sets: the header of include/mprime_panel.h says they are one rule."""
    from multiprime_amd.validate import amplicons
    rng = np.random.default_rng(5)
    for _ in range(300):
        lo, hi = int(rng.integers(0, 40)), int(rng.integers(40, 120))
        f = {int(p): "f%d" % p for p in rng.integers(0, 300, rng.integers(1, 12))}
        r = {int(p): "r%d" % p for p in rng.integers(0, 300, rng.integers(1, 12))}
        assert panel.pcr_products(f, r, lo, hi) == amplicons(f, r, lo, hi) == R.join(f, r, lo, hi)


# ---- what the device receives -----------------------------------------------------------------------------------------------------------
def test_loss_table_against_direct_evaluation():
    t = panel.loss_table()
    assert t.shape == (65, 65, 64) and t.dtype == np.uint8
    for l in range(65):
        for gc in range(65):
            for d2 in range(64):
                want = 1 <= l and gc <= l and R.loss(l, gc, 0, d2) > 3
                assert t[l, gc, d2] == want, (l, gc, d2)
    assert t[7, 4, 23] == 0 and t[7, 6, 23] == 1                            # the two 7-base ends of the plain fixture's history


def device_delta_g(end, p):
    """dm_delta_g of csrc/dimer.hip on the host: the same additions in the same order."""
    idx = {"A": 0, "C": 1, "G": 2, "T": 3}
    g = 0.0
    for n in range(1, len(end)):
        g = g + p[idx[end[n]] * 4 + idx[end[n - 1]]]
    g = g + p[16 + (idx[end[0]] * 4 + idx[end[-1]]) * 2 + (end[-2:] == "TA")]
    g = g + -p[48 + len(end)]
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    half = len(end) // 2
    if len(end) % 2 == 0 and all(end[t] == comp[end[half + t]] for t in range(half)):
        g = g + p[48 + 64 + 1]
    return g


def test_dg_params_against_the_references_expression():
    p = panel.dg_params().tolist()               # Python floats: numpy's round() is not CPython's
    from multiprime_amd.dimer import dg_limit
    limit = dg_limit()
    ends = {"GCTA", "ACGT", "GGATCC", "TA", "A", "GCGCATT"}                       # a TA end, self-complementary ends, the shortest
    for case in ("plain", "degenerate"):
        for path in ("core.fa", "new.fa"):
            for seq in R.parse_primers(os.path.join(PANEL, case, path)):
                for l, _, e in R.ends_of(seq):
                    ends.add(e)
    assert len(ends) > 300
    for e in sorted(ends):
        g = device_delta_g(e, p)
        assert round(g, 2) == R.delta_g(e) == panel.delta_g(e), e
        assert (g < limit) == (R.delta_g(e) < -5), e
    assert not any(p[48:])


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_flags_and_defaults():
    o, _ = panel.parse_args(["-c", "a", "-n", "b", "-o", "c"])
    assert (o.core, o.new, o.ref, o.size, o.len, o.seedmms, o.proc, o.func, o.out) == ("a", "b", None, "150,2000", 9, 1, 10, "DO", "c")
    o, _ = panel.parse_args(["--core", "a", "--new", "b", "--ref", "r", "--size", "1,2", "--len", "0", "--seedmms", "3", "--proc", "2",
                             "--func", "D", "--out", "c"])
    assert (o.ref, o.size, o.len, o.seedmms, o.proc, o.func) == ("r", "1,2", 0, 3, 2, "D")


@pytest.mark.parametrize("argv, text", [([], "Usage"), (["-n", "b", "-o", "c"], "Core primer file must be specified !!!"),
                                        (["-c", "a", "-o", "c"], "New primer file must be specified !!!"),
                                        (["-c", "a", "-n", "b"], "No output file provided !!!")])
def test_missing_flags_exit_1(capsys, argv, text):
    with pytest.raises(SystemExit) as e:
        panel.parse_args(argv)
    assert e.value.code == 1 and text in capsys.readouterr().out


def test_errors_are_named_before_anything_runs(tmp_path):
    good = tmp_path / "good.fa"
    good.write_text(">g\nACGTACGTACGTAC\n")

    def fa(name, seq):
        p = tmp_path / name
        p.write_text(">x\n" + seq + "\n")
        return str(p)
    with pytest.raises(ValueError, match="65 bases"):
        panel.Dimer(fa("long.fa", "A" * 65), str(good), str(tmp_path / "o"))
    with pytest.raises(ValueError, match="IUPAC"):
        panel.Dimer(str(good), fa("bad.fa", "ACGTXACGT"), str(tmp_path / "o"))
    with pytest.raises(ValueError, match="-m 4"):
        panel.off_targets(str(good), str(good), 4, 9, "ref.fa", "150,2000", str(tmp_path / "o")).run()
    with pytest.raises(ValueError, match="3 bases after -l 3"):
        panel.off_targets(str(good), str(good), 1, 3, "ref.fa", "150,2000", str(tmp_path / "o")).run()
    with pytest.raises(ValueError, match="needs -r"):
        panel.off_targets(str(good), str(good), 1, 9, "", "150,2000", str(tmp_path / "o")).run()
    with pytest.raises(ValueError, match="needs -r"):                        # through main(): refused before the dimer step
        panel.main(["-c", str(good), "-n", str(good), "-o", str(tmp_path / "o")])
    assert sorted(os.listdir(tmp_path)) == ["bad.fa", "good.fa", "long.fa"]  # nothing was written


def test_script_is_a_pass_through():
    src = open(os.path.join(REPO, "scripts", "Primer_set_update.py")).read()
    assert "multiprime_amd.panel" in src and "import pickle" not in src
    assert "import pickle" not in open(panel.__file__).read()               # no cache found on disk is ever unpickled
