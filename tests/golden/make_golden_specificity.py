#!/usr/bin/env python3
"""Golden vectors for SURVEY §8f-3, the off-target half (scripts/primer_specificity.py): everything the script does AROUND the mapper,
recorded from the unmodified reference class.  bowtie2 / samtools are not installed here, but the script maps only when
<primers>.for.sam / .rev.sam exist already (bowtie_map), so the cases hand it SAM text and record what it writes: <out>, <out>.pair.num,
<out>.total.acc.num (PCR_product and the writers of run) and <primers>.term.fa (get_term).  Beside them, what its optparse command
line (argsParse) makes of a few argument lists.

The hand-written cases cover: several genes; many reads at one start (the last line wins); an empty forward / reverse strand; the
whole-gene reject on either side; the first start without a reverse site ending the gene's search; products of exactly size_lo and
size_hi (both left out) and one base inside them.  The seeded cases are make_golden_validate.py's generator.

The reference walks the genes with products in the order of a Python set (random from one process to the next).  So that the
recorded files pin that order too, the forward SAM lines of a case are put in the order the reference printed its genes (the
lines of one gene keep their order), and the reference is run again on the reordered text: the files it writes then are recorded,
and they list the genes in order of their first forward line — the drop-in's order.   Run:  python tests/golden/make_golden_specificity.py"""
import contextlib
import gzip
import importlib.util
import io
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/scripts/primer_specificity.py"
sys.path.insert(0, HERE)
from make_golden_validate import random_case, sam_line  # noqa: E402


def load_reference():
    spec = importlib.util.spec_from_file_location("primer_specificity_ref", REF)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["primer_specificity_ref"] = mod          # the class is pickled for the reference's worker pool
    spec.loader.exec_module(mod)
    return mod


def md(n):
    return ["AS:i:0", "XN:i:0", "NM:i:0", f"MD:Z:{n}", "YT:Z:UU"]


def hand_cases():
    primers = [("PF", "ACGTTGCAAGGCTTACGA"), ("PR", "TTGACCGGTAACGTCAGT"), ("QF", "GGATCCATGCAAGCTTAC"), ("QR", "CCGGAATTCGGTACCTTA"),
               ("SF", "AATTCCGGAATTCCGGTT")]
    f, r = [], []
    # g1: several starts, one of them hit by four reads (the last line wins); products of length size_lo - 1 .. size_lo + 1 and
    # size_hi - 1 .. size_hi + 1 around start 1000
    f += [sam_line(name, 0, "g1", 1001, 18, md(18)) for name in ("PF_0", "QF_0", "SF_0", "QF_0")]
    f += [sam_line("PF_0", 0, "g1", 1003, 18, md(18)), sam_line("SF_0", 0, "g1", 1500, 18, md(18))]
    r += [sam_line("PR_0", 16, "g1", 1000 + lo_len, 18, md(18)) for lo_len in (99, 100, 101)]           # stop = 1000 + L - 1 + 1 (1-based)
    r += [sam_line("QR_0", 16, "g1", 1000 + hi_len, 18, md(18)) for hi_len in (1499, 1500, 1501)]
    # g2: the first dead start — 3000 has no stop in range, so 5000 (which has one at 5300) gives nothing
    f += [sam_line("PF_0", 0, "g2", 101, 18, md(18)), sam_line("QF_0", 0, "g2", 3001, 18, md(18)), sam_line("PF_0", 0, "g2", 5001, 18, md(18))]
    r += [sam_line("PR_0", 16, "g2", 401, 18, md(18)), sam_line("QR_0", 16, "g2", 5301, 18, md(18))]
    # g3: whole-gene reject, the stops too far right of every start; g4: the stops too close to every start
    f += [sam_line("PF_0", 0, "g3", 11, 18, md(18)), sam_line("QF_0", 0, "g3", 21, 18, md(18))]
    r += [sam_line("PR_0", 16, "g3", 5001, 18, md(18))]
    f += [sam_line("PF_0", 0, "g4", 501, 18, md(18))]
    r += [sam_line("PR_0", 16, "g4", 531, 18, md(18)), sam_line("QR_0", 16, "g4", 400, 18, md(18))]
    # g5: reverse only; g6: forward only; g7: a plain pair, with a site the MD rule drops (mismatch in the last two bases)
    r += [sam_line("PR_0", 16, "g5", 700, 18, md(18))]
    f += [sam_line("PF_0", 0, "g6", 700, 18, md(18))]
    f += [sam_line("SF_0", 0, "g7", 51, 18, md(18)), sam_line("QF_0", 0, "g7", 52, 18, ["AS:i:-6", "NM:i:1", "MD:Z:16A1"])]
    r += [sam_line("PR_0", 16, "g7", 351, 18, md(18)), sam_line("QR_0", 16, "g7", 352, 18, ["AS:i:-6", "NM:i:1", "MD:Z:3C14"])]
    base = {"primers": primers, "term_len": 0, "term_threshold": 4, "size": "100,1500", "targets": None}
    return [dict(base, name="hand", for_sam="".join(f), rev_sam="".join(r)),
            dict(base, name="hand_no_reverse", for_sam="".join(f), rev_sam=""),
            dict(base, name="hand_no_forward", for_sam="", rev_sam="".join(r)),
            dict(base, name="hand_narrow", for_sam="".join(f), rev_sam="".join(r), size="50,400", term_threshold=2)]


def run_case(mod, case):
    with tempfile.TemporaryDirectory() as td:
        pf = os.path.join(td, "primers.fa")
        open(pf, "w").write("".join(f">{n}\n{s}\n" for n, s in case["primers"]))
        open(os.path.join(td, "primers.for.sam"), "w").write(case["for_sam"])
        open(os.path.join(td, "primers.rev.sam"), "w").write(case["rev_sam"])
        out = os.path.join(td, "spec.out")
        app = mod.off_targets(primer_file=pf, term_length=case["term_len"], reference_file=os.path.join(td, "unused.fa"), mismatch_num=1,
                              term_threshold=case["term_threshold"], bowtie="bowtie2", PCR_product_size=case["size"], outfile=out, nproc=2)
        with contextlib.redirect_stdout(io.StringIO()):
            app.run()
        return {"term_fa": open(os.path.join(td, "primers.term.fa")).read(), "out": open(out).read(),
                "pair_num": open(out + ".pair.num").read(), "total_acc_num": open(out + ".total.acc.num").read()}


def in_output_order(sam, out):
    """The SAM lines regrouped so that the genes of <out> come first, in <out>'s order; a gene's lines keep their order."""
    order = {}
    for line in out.splitlines()[1:]:
        order.setdefault(line.split("\t")[0], len(order))
    lines = sam.splitlines(True)
    return "".join(sorted(lines, key=lambda ln: order.get(ln.split("\t")[2], len(order))))


def record(mod, case):
    for _ in range(4):
        got = run_case(mod, case)
        regrouped = in_output_order(case["for_sam"], got["out"])
        if regrouped == case["for_sam"]:
            return got
        case["for_sam"] = regrouped
    raise RuntimeError(f"{case['name']}: the reference's gene order does not settle")


ARGVS = [["-i", "p.fa", "-r", "bg.fa", "-o", "out"],
         ["-i", "p.fa", "-r", "bg.fa", "-o", "out", "-l", "9", "-t", "3", "-s", "50,300", "-p", "4", "-b", "bowtie", "-m", "0"],
         ["--input", "p.fa", "--ref", "bg.fa", "--out", "out", "--len", "12", "--term", "0", "--s", "80,900", "--proc", "1", "--seedmms", "2"],
         ["-i", "p.fa", "-o", "out"],
         ["-r", "bg.fa", "-o", "out"],
         ["-i", "p.fa", "-r", "bg.fa"],
         []]


def parses(mod):
    out = []
    for argv in ARGVS:
        saved = sys.argv
        sys.argv = ["primer_specificity.py"] + argv
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                options, args = mod.argsParse()
            out.append({"argv": argv, "options": vars(options), "args": args, "exit": None})
        except SystemExit as e:
            out.append({"argv": argv, "options": None, "args": None, "exit": e.code})
        finally:
            sys.argv = saved
    return out


def main():
    mod = load_reference()
    cases = hand_cases()
    for seed, args in ((11, (0, 4, "100,1500", 12, 400)), (12, (8, 4, "150,1200", 6, 260)), (13, (12, 6, "50,400", 25, 500)),
                       (14, (0, 0, "100,1500", 40, 120))):
        case = random_case(seed, *args, False)
        case["name"] = f"rand{seed}"
        cases.append(case)
    for case in cases:
        case["recorded"] = record(mod, case)
        print(case["name"], {k: len(v.splitlines()) for k, v in case["recorded"].items()})
    data = {"cases": cases, "parses": parses(mod)}
    open(os.path.join(HERE, "specificity.json.gz"), "wb").write(gzip.compress(json.dumps(data, sort_keys=True).encode(), 9, mtime=0))


if __name__ == "__main__":
    main()
