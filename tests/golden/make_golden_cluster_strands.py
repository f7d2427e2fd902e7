#!/usr/bin/env python3
"""Goldens for the .clstr layout of a both-strand clustering (`at +/dd.dd%` / `at -/dd.dd%` member lines): the mixed set of
tests/strand_cases.py is clustered at 0.8 by the plain restatement of the both-strand rule (tests/strand_ref.py; the device writes the same
bytes, tests/test_strand_gpu.py), and the UNMODIFIED reference's extract_cluster script (imported by path) consumes the FASTA and the
.clstr.  Stored: the input, our .clstr, and the reference's cluster.txt and cluster.identities.txt — they pin that the reference reads
the signed lines and sees the same members and identity strings.
Usage: python tests/golden/make_golden_cluster_strands.py <reference>/scripts/extract_cluster_V4.py   -> tests/golden/cluster_strands.*.gz"""
import gzip
import importlib.util
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import cluster_cases  # noqa: E402
import strand_cases as cases  # noqa: E402
import strand_ref as ref  # noqa: E402


def put(name, text):
    with open(os.path.join(HERE, name), "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
        g.write(text.encode())


def main(script):
    spec = importlib.util.spec_from_file_location("extract_cluster", script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    records = cases.mixed_set()
    ids, seqs = [i for i, _ in records], [s for _, s in records]
    fa = cluster_cases.fasta(records)
    clstr = ref.clstr_text(ids, seqs, *ref.cluster(seqs, identity_permille=800))
    with tempfile.TemporaryDirectory() as td:
        paths = {k: os.path.join(td, k) for k in ("in.fa", "in.clstr", "cluster.txt", "cluster.identities.txt", "Cluster_fa")}
        open(paths["in.fa"], "w").write(fa)
        open(paths["in.clstr"], "w").write(clstr)
        mod.Extract_Cluster(Sequence_file=paths["in.fa"], Cluster_file=paths["in.clstr"], Outfile=paths["cluster.txt"],
                            Identity_file=paths["cluster.identities.txt"], Seq_number=500, Cluster_fa=paths["Cluster_fa"], nproc=1).run()
        txt, identities = open(paths["cluster.txt"]).read(), open(paths["cluster.identities.txt"]).read()
    put("cluster_strands.fa.gz", fa)
    put("cluster_strands.clstr.gz", clstr)
    put("cluster_strands.txt.gz", txt)
    put("cluster_strands.identities.txt.gz", identities)
    print(len(ids), "records,", clstr.count(">Cluster"), "clusters,", clstr.count("at -/"), "minus-strand members")


if __name__ == "__main__":
    main(sys.argv[1])
