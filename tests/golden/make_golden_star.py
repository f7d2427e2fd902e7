#!/usr/bin/env python3
"""Fixtures of the star-alignment tests: the reference workflow's own cluster as its mafft step read and wrote it — data of the
reference's test run, no program text.  Stored gzipped (mtime 0) under tests/golden/inputs/:
    Cluster_0_20727.tfa    500 unaligned records of 1698..1867 bases, IUPAC letters present
    Cluster_0_20727.tmsa   mafft's alignment of them: width 1951, 1702 majority columns
Usage: python tests/golden/make_golden_star.py <reference>/test_data/results   (an existing identical fixture is left as it is)"""
import gzip
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from anchor_ref import anchor_of  # noqa: E402


def records(raw):
    out = []
    for line in raw.decode().splitlines():
        if line.startswith(">"):
            out.append([line.split()[0], ""])
        elif line.strip():
            out[-1][1] += line.strip()
    return out


def put(name, raw):
    path = os.path.join(HERE, "inputs", name + ".gz")
    if os.path.exists(path) and gzip.open(path).read() == raw:
        return "kept"
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
        g.write(raw)
    assert os.path.getsize(path) < 1 << 20
    return "written"


def main(results):
    tfa = open(os.path.join(results, "Clusters_fa", "Cluster_0_20727.tfa"), "rb").read()
    tmsa = open(os.path.join(results, "Clusters_msa", "Cluster_0_20727.tmsa"), "rb").read()
    fa, msa = records(tfa), records(tmsa)
    lens = [len(s) for _, s in fa]
    assert len(fa) == 500 and (min(lens), max(lens)) == (1698, 1867) and any(ch not in "ACGT" for _, s in fa for ch in s.upper())
    assert sorted(i for i, _ in fa) == sorted(i for i, _ in msa) and {len(s) for _, s in msa} == {1951}
    assert {i: s.upper() for i, s in fa} == {i: s.upper().replace("-", "") for i, s in msa}
    assert len(anchor_of([s for _, s in msa])[0]) == 1702
    print("Cluster_0_20727.tfa", put("Cluster_0_20727.tfa", tfa), "/ Cluster_0_20727.tmsa", put("Cluster_0_20727.tmsa", tmsa))


if __name__ == "__main__":
    main(sys.argv[1])
