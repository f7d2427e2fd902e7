#!/usr/bin/env python3
"""Golden for the read-to-primer assignment: what the UNMODIFIED reference scripts write for the synthetic run of
tests/ont_cases.golden_reads.  FindONTprimerV3.py runs as a subprocess on the run as fq, fq.gz, fa and fa.gz, FindONTexpandprimer.py on
the fq file, each from a working directory that holds relative file names (the expand file's name rule shows only there).  Stored in
ont_small.json.gz: the input texts, and per case the command's flags, the .num lines and the expand file's name and text.  Data only.
Usage: python tests/golden/make_golden_ont.py <reference>/scripts   -> tests/golden/ont_small.json.gz"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ont_cases as cases  # noqa: E402

PRIMER_FILE = "fa_panel.fa"                    # str.strip("fa") takes letters from both ends: the expand file is _panel.expand.fa
CASES = [("v3_fq", "FindONTprimerV3.py", "reads.fq", "fq"), ("v3_fq_gz", "FindONTprimerV3.py", "reads.fq.gz", "fq"),
         ("v3_fa", "FindONTprimerV3.py", "reads.fa", "fa"), ("v3_fa_gz", "FindONTprimerV3.py", "reads.fa.gz", "fa"),
         ("expand_fq", "FindONTexpandprimer.py", "reads.fq", "fq")]


def main(scripts):
    reads = cases.golden_reads()
    texts = {"reads.fq": cases.fastq_text(reads), "reads.fa": cases.fasta_text(reads)}
    out = {"primers": cases.PRIMERS, "primer_file": PRIMER_FILE, "inputs": texts, "length": cases.LENGTH, "cases": {}}
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, PRIMER_FILE), "w") as f:
            f.write(cases.PRIMERS)
        for name, text in texts.items():
            with open(os.path.join(td, name), "w") as f:
                f.write(text)
            with gzip.open(os.path.join(td, name + ".gz"), "wb") as f:
                f.write(text.encode())
        for case, script, reads_file, fmt in CASES:
            before = set(os.listdir(td))
            flags = ["-i", reads_file, "-s", PRIMER_FILE, "-p", "2", "-l", str(cases.LENGTH), "-f", fmt, "-o", case]
            subprocess.run([sys.executable, os.path.join(scripts, script)] + flags, cwd=td, check=True, stdout=subprocess.DEVNULL)
            new = sorted(set(os.listdir(td)) - before - {case + ".num"})
            expand_file = new[0] if new else "_panel.expand.fa"
            out["cases"][case] = {"script": script, "flags": flags, "lines": open(os.path.join(td, case + ".num")).readlines(),
                                  "expand_file": expand_file, "expand_text": open(os.path.join(td, expand_file)).read()}
    path = os.path.join(HERE, "ont_small.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, indent=0, sort_keys=True).encode())
    print(path, os.path.getsize(path), "bytes;", {k: len(v["lines"]) - 1 for k, v in out["cases"].items()}, "pairs")


if __name__ == "__main__":
    main(sys.argv[1])
