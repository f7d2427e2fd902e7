"""Writes tests/golden/setscreen/: a candidate file, a background and the three files a run with -r writes for them (maximal
mode, the defaults: -p 150,2000 -d 12 --seedmms 1 --max-offtarget 0), plus the .next.xls, and as plain.* what a run without -r writes.

No reference script can write these (get_Maxprimerset_V3.py does not run), so the pair counts come from the model of the rule,
tests/setscreen_ref.py, injected into the set cover (OffTargetExaminer(table=...)); the dimer test runs on the CPU checker library
as in the other set-cover fixtures.  The fixture pins the model: tests/test_setscreen.py recomputes it, tests/test_setscreen_gpu.py
compares the device path with it.

    python tests/golden/make_golden_setscreen.py
"""
import contextlib
import io
import os
import subprocess
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import setscreen_cases as cases          # noqa: E402
import setscreen_ref as ref              # noqa: E402
from multiprime_amd import maxset        # noqa: E402
from multiprime_amd._abi import Library  # noqa: E402
from multiprime_amd.setscreen import OffTargetExaminer  # noqa: E402


def main():
    subprocess.check_call(["make", "-C", os.path.join(REPO, "oracle")], stdout=subprocess.DEVNULL)
    lib = Library(os.path.join(REPO, "oracle", "_build", "libmprime_oracle.so"))
    rows, clusters = cases.golden_case()
    table = ref.pair_table(ref.sites(rows, cases.all_primers(clusters), cases.DIST, 1), 150, 2000)
    out_dir = os.path.join(HERE, "setscreen")
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        inp, out = os.path.join(td, "candidates.txt"), os.path.join(td, "final.xls")
        with open(inp, "w") as f:
            f.write(cases.candidate_text(clusters))
        opts = types.SimpleNamespace(input=inp, step=5, method="T", out=out, device=0, max_offtarget=0, cross_only=False, lookahead=4)
        with contextlib.redirect_stdout(io.StringIO()):
            maxset.run(opts, library=lib, offtarget=OffTargetExaminer(table=table))
        keep = {"candidates.txt": inp, "final.xls": out, "final.xls.offtarget.tsv": out + ".offtarget.tsv",
                "final.xls.offtarget.set.tsv": out + ".offtarget.set.tsv", "fina.next.xls": out.rstrip(".xls") + ".next.xls"}      # (the script strips characters, not the suffix)
        for name, path in keep.items():
            with open(path) as f, open(os.path.join(out_dir, name), "w") as g:
                g.write(f.read())
        # the same candidates without -r: what the set cover writes today
        with contextlib.redirect_stdout(io.StringIO()):
            maxset.run(types.SimpleNamespace(input=inp, step=5, method="T", out=out, device=0), library=lib)
        for name, path in (("plain.final.xls", out), ("plain.fina.next.xls", out.rstrip(".xls") + ".next.xls")):
            with open(path) as f, open(os.path.join(out_dir, name), "w") as g:
                g.write(f.read())
    with open(os.path.join(out_dir, "background.fa"), "w") as f:
        f.write(cases.fasta_text(rows))
    log = open(os.path.join(out_dir, "final.xls.offtarget.tsv")).read()
    assert "rejected" in log and "selected" in log
    print(log)
    print(open(os.path.join(out_dir, "final.xls.offtarget.set.tsv")).read())


if __name__ == "__main__":
    main()
