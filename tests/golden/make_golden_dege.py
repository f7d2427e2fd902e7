#!/usr/bin/env python3
"""Goldens of the DegePrime drop-ins (scripts/TrimAlignment.py, scripts/run_dege.py), produced by RUNNING the unmodified Perl scripts
DEGEPRIME-1.1.0/TrimAlignment.pl and DegePrime.pl of the reference:
    dege_sub    rows 0..149, columns 400..719 of test_data/1000_fasta.msa: the slice, its trim at the default flags, one table (-l 18 -d 12)
    dege_wide   all 1000 rows, columns 560..649: the trim and the NumberMatching column of three runs (-l 18 -d 24 -skip 5)
    small       the hand-made alignment of tests/dege_cases.py: its trim at five flag sets and the table of one lower-case output
Usage: python tests/golden/make_golden_dege.py <reference>   -> tests/golden/dege.json.gz"""
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import dege_cases as cases  # noqa: E402


def read_fasta(path):
    out = []
    for line in open(path):
        line = line.rstrip("\n")
        if line.startswith(">"):
            out.append([line[1:].split()[0], []])
        elif out:
            out[-1][1].append(line)
    return [(i, "".join(s)) for i, s in out]


def perl(script, args, cwd):
    t0 = time.time()
    p = subprocess.run(["perl", script] + args, cwd=cwd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f"{script} {args}: status {p.returncode}\n{p.stderr[-2000:]}")
    return time.time() - t0


def main():
    ref = sys.argv[1]
    dp = os.path.join(ref, "scripts", "DEGEPRIME-1.1.0")
    trim_pl, dege_pl = os.path.join(dp, "TrimAlignment.pl"), os.path.join(dp, "DegePrime.pl")
    msa = read_fasta(os.path.join(ref, "test_data", "1000_fasta.msa"))
    g = {}
    with tempfile.TemporaryDirectory() as td:
        def trim(text, flags):
            open(os.path.join(td, "in.fa"), "w").write(text)
            perl(trim_pl, ["-i", "in.fa", "-o", "out.fa"] + flags, td)
            return open(os.path.join(td, "out.fa")).read()

        def dege(text, flags):
            open(os.path.join(td, "trim.fa"), "w").write(text)
            sec = perl(dege_pl, ["-i", "trim.fa", "-o", "table.txt"] + flags, td)
            return open(os.path.join(td, "table.txt")).read(), sec

        sub = "".join(">%s\n%s\n" % (i, s[400:720]) for i, s in msa[:150])
        sub_trim = trim(sub, [])
        f = cases.SUB_FLAGS
        table, sec = dege(sub_trim, ["-l", str(f["l"]), "-d", str(f["d"])])
        g["dege_sub"] = {"input": sub, "trim": sub_trim, "flags": f, "table": table, "perl_seconds": round(sec, 1)}
        print("dege_sub", len(table.splitlines()) - 1, "windows", round(sec, 1), "s")

        wide = "".join(">%s\n%s\n" % (i, s[560:650]) for i, s in msa)
        wide_trim = trim(wide, [])
        f = cases.WIDE_FLAGS
        runs = []
        for _ in range(3):
            table, sec = dege(wide_trim, ["-l", str(f["l"]), "-d", str(f["d"]), "-skip", str(f["skip"])])
            runs.append([int(line.split("\t")[6]) for line in table.splitlines()[1:]])
            print("dege_wide", len(runs[-1]), "windows, total", sum(runs[-1]), round(sec, 1), "s")
        g["dege_wide"] = {"trim": wide_trim, "flags": f, "table": table, "matching": runs}

        small = cases.small_fasta()
        g["small"] = {"input": small, "trims": {name: {"flags": flags, "text": trim(small, flags)} for name, flags in cases.TRIMS.items()}}
        of, flags = cases.SMALL_TABLE
        g["small"]["table"] = {"of": of, "flags": flags, "text": dege(g["small"]["trims"][of]["text"], flags)[0]}
        for name, t in g["small"]["trims"].items():
            print("small", name, len(t["text"].splitlines()[1]), "columns")
    open(os.path.join(HERE, "dege.json.gz"), "wb").write(gzip.compress(json.dumps(g, sort_keys=True).encode(), 9, mtime=0))


if __name__ == "__main__":
    main()
