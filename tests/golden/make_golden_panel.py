#!/usr/bin/env python3
"""Fixtures of the panel update (tests/golden/panel/<case>/): small primer FASTAs, hand-written .sam/.for.sam/.rev.sam triplets, and
the four files the UNMODIFIED reference script scripts/Primer_set_update.py writes for them — <out>.dimer, <out>.dimer.dimer_num (-f D)
and <out>.offtargets, <out>.offtargets.num (-f O; with the three SAM files of each input present the script maps nothing).  Data only.

    python tests/golden/make_golden_panel.py /path/to/reference/scripts/Primer_set_update.py

The script runs in a scratch directory (it pickles .primer_set and writes .gene_position caches beside its inputs: those are not
recorded).  Its line order comes from a process pool and from Python sets, so the tests compare sorted lines (.dimer), per-gene blocks
(.offtargets) and sets of lines (the two count files).

Cases
  plain       4 core + 9 new records without degenerate letters, one sequence common to both files (its line comes out twice), one
              sequence repeated inside the new file under two names (first position, last name); hits by Loss at d2 = 0, by Loss at
              d2 > 0, and by deltaG alone at d2 >= 21 (the branch finDimer does not have); a 4-base and a 19-base primer.
  degenerate  degenerate letters only where the reference's output does not depend on string hashing: in partners, and in a primer's 5'
              part beyond its 18-base end.
  sam         -f O: core and new SAM triplets over four genes — a start claimed by several reads of one file (the last line wins) and by
              both files, MD:Z values ending in runs of 4 and 5 and in "10" read as 10 / "0" read as 0, both whole-gene early outs,
              the first start without a stop ending a gene, lengths equal to the bounds (-s 100,1500), products in all three joins on
              one gene.
"""
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "panel")
COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(COMP)[::-1]


def fasta(records):
    return "".join(f">{n}\n{s}\n" for n, s in records)


def dimer_cases():
    c1 = "ATGGCTAGCTTAGGACCTGA"
    c2 = "TTGACCATGCAAGTCCGATG"
    c3 = "CAGTTACGGATCCATAGCAA"
    shared = "GGATACCTTGAGCAATCGTA"
    # n1: its last 8 bases pair with the 3' end of c1 (d2 = 0); n2: its last 7 bases pair inside c2, 6 bases from its 3' end
    n1 = "ACCTATGCAATG" + rc(c1[-8:])
    n2 = "TGCATTAGACCAT" + rc(c2[-13:-6])
    # n3 (30 bases) starts with RC of the 7-base end of n4: d2 = 23 for n4 -> n3, a hit by deltaG alone
    end7 = "GCGCATT"
    n4 = "ATTACATTCAATA" + end7
    n3 = rc(end7) + "ATATTAATTATATTTAATATTAT"
    n5 = "TTACAATCATAC" + rc(shared[-8:])        # pairs with the common sequence: its job runs once per file and prints the line twice
    plain = {
        "core": [("c1", c1), ("c2", c2), ("c3", c3), ("shared_core", shared)],
        "new": [("n1", n1), ("n2", n2), ("n3", n3), ("shared_new", shared), ("n4", n4), ("n1_again", n1), ("tiny", "GCGC"),
                ("n19", "TACATTTAACATTAAT" + "GGC"), ("n5", n5)],
    }
    d_core = "RTGGCTAGCTTAGGACCTGA"                 # degenerate at its 5' end, 20 bases: no end reaches position 0
    degenerate = {
        "core": [("d1", d_core), ("d2", "TTGACCAYGCAAGTCCGATG"), ("d3", "ACGTTGCANNTTGACCAATG")],
        "new": [("e1", "ACCTATGCAATG" + rc(d_core[-8:])), ("e2", "NRACCTATGCAATTCAATGCATTGGTCAA"), ("e3", "TTTTCATCGGACTTGCGTGG")],
    }
    return {"plain": plain, "degenerate": degenerate}


def sam_line(read, flag, gene, pos1, md, length=9):
    return "\t".join([read, str(flag), gene, str(pos1), "255", f"{length}M", "*", "0", "0", "A" * length, "I" * length, "XA:i:0", f"MD:Z:{md}",
                      "NM:i:0"]) + "\n"


def sam_case():
    core = [("cA", "ATGGCTAGCTTAGGACCTGA"), ("cB", "TTGACCATGCAAGTCCGATG")]
    new = [("nA", "CAGTTACGGATCCATAGCAA"), ("nB", "GGATACCTTGAGCAATCGTA"), ("nC", "ACCTATGCAATGTCAGGTCC")]
    cf, cr, nf, nr = [], [], [], []
    # g1: products in all three joins; start 1000 claimed by three core reads (the last line wins) and by a new read as well
    cf += [sam_line(r, 0, "g1", 1001, "9") for r in ("cA_0", "cB_0", "cA_0|>cB_0")]
    cf += [sam_line("cB_0", 0, "g1", 1003, "9")]
    nf += [sam_line("nA_0", 0, "g1", 1001, "9"), sam_line("nB_0", 0, "g1", 1201, "9")]
    # lengths 99, 100, 101 and 1499, 1500, 1501 from start 1000 (stop = start + length - 1, 1-based + 1)
    nr += [sam_line("nC_0", 16, "g1", 1000 + n, "9") for n in (99, 100, 101, 1499, 1500, 1501)]
    cr += [sam_line("cA_0", 16, "g1", 1601, "9"), sam_line("cB_0", 16, "g1", 1300, "9")]
    # MD:Z endings: "4" and "3A4" are dropped, "5" and "3A5" kept, "10" reads as 10, "9A0" as 0
    cf += [sam_line("cA_0", 0, "g2", 101, "4"), sam_line("cA_0", 0, "g2", 111, "3A4"), sam_line("cB_0", 0, "g2", 121, "3A5"),
           sam_line("cB_0", 0, "g2", 131, "9A0", 10)]
    nr += [sam_line("nA_0", 16, "g2", 401, "5"), sam_line("nB_0", 16, "g2", 411, "10", 10)]
    # g3: the first start without a stop ends the gene — 3000 has none, 5000 would have 5300
    nf += [sam_line("nA_0", 0, "g3", 101, "9"), sam_line("nB_0", 0, "g3", 3001, "9"), sam_line("nC_0", 0, "g3", 5001, "9")]
    nr += [sam_line("nA_0", 16, "g3", 401, "9"), sam_line("nB_0", 16, "g3", 5301, "9")]
    cr += [sam_line("cA_0", 16, "g3", 451, "9")]
    # g4: whole-gene early out, every stop too far right (core F x new R); g5: every stop too close (new F x core R)
    cf += [sam_line("cA_0", 0, "g4", 11, "9"), sam_line("cB_0", 0, "g4", 21, "9")]
    nr += [sam_line("nC_0", 16, "g4", 5001, "9")]
    nf += [sam_line("nC_0", 0, "g5", 501, "9")]
    cr += [sam_line("cB_0", 16, "g5", 531, "9"), sam_line("cA_0", 16, "g5", 400, "9")]
    # g6: forward sites only (no join has both sides)
    cf += [sam_line("cA_0", 0, "g6", 11, "9")]
    nf += [sam_line("nA_0", 0, "g6", 11, "9")]
    return {"core": core, "new": new, "core.for.sam": "".join(cf), "core.rev.sam": "".join(cr), "new.for.sam": "".join(nf),
            "new.rev.sam": "".join(nr), "core.sam": "@HD\tVN:1.0\n", "new.sam": "@HD\tVN:1.0\n"}


def run_reference(script, case_dir, func, extra=()):
    """The reference on a copy of the case's inputs; its outputs (prefix `out`) are copied back into case_dir."""
    with tempfile.TemporaryDirectory() as td:
        for name in os.listdir(case_dir):
            if not name.startswith("out."):
                shutil.copy(os.path.join(case_dir, name), td)
        cmd = [sys.executable, script, "-c", os.path.join(td, "core.fa"), "-n", os.path.join(td, "new.fa"), "-f", func, "-p", "2",
               "-o", os.path.join(td, "out")] + list(extra)
        r = subprocess.run(cmd, cwd=td, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"the reference failed on {case_dir}:\n{r.stdout}\n{r.stderr}")
        made = [n for n in os.listdir(td) if n.startswith("out.")]
        for name in made:
            shutil.copy(os.path.join(td, name), case_dir)
        return sorted(made)


def main():
    if len(sys.argv) != 2 or not os.path.exists(sys.argv[1]):
        raise SystemExit(__doc__)
    script = os.path.abspath(sys.argv[1])
    for name, case in dimer_cases().items():
        d = os.path.join(OUT, name)
        os.makedirs(d, exist_ok=True)
        for side in ("core", "new"):
            with open(os.path.join(d, side + ".fa"), "w") as f:
                f.write(fasta(case[side]))
        print(name, run_reference(script, d, "D"))
    case = sam_case()
    d = os.path.join(OUT, "sam")
    os.makedirs(d, exist_ok=True)
    for key, value in case.items():
        with open(os.path.join(d, key + (".fa" if key in ("core", "new") else "")), "w") as f:
            f.write(fasta(value) if key in ("core", "new") else value)
    print("sam", run_reference(script, d, "O", ["-s", "100,1500"]))


if __name__ == "__main__":
    main()
