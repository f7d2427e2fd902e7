#!/usr/bin/env python3
"""Golden for the host side of the identity merge: what the UNMODIFIED reference scripts decide and do to a small Clusters_fa tree.
The tree comes from the reference's extract_cluster script (imported by path) on a .clstr written by tests/cluster_ref.clstr_text for
the planted clusters of tests/ani_cases.golden_clusters.  The reference's merge_cluster_by_ANI script then runs as a subprocess with
-p 1, once with -d T and once with -d F, with a stand-in `fastANI` ahead on PATH: it prints the reported pairs of the rule's plain
restatement (tests/ani_ref.py, s = 1024, floor 0.7) in fastANI's five columns, identity in percent.  Stored in ani_small.json.gz: the
input tree, and per mode history.txt and the resulting tree (every file's bytes).
Usage: python tests/golden/make_golden_ani.py <reference>/scripts   -> tests/golden/ani_small.json.gz"""
import gzip
import importlib.util
import json
import os
import stat
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)

import ani_cases as cases  # noqa: E402
import ani_ref as ref  # noqa: E402
import cluster_ref  # noqa: E402

STAND_IN = """#!%s
import sys
sys.path.insert(0, %r)
import ani_ref as ref
a = sys.argv[1:]
ql, rl, out = a[a.index("--ql") + 1], a[a.index("--rl") + 1], a[a.index("-o") + 1]
files = lambda p: [x.strip() for x in open(p) if x.strip()]
sk = lambda p: ref.sketch(ref.read_fasta(p)[0][1], 1024)
with open(out, "w") as f:
    for q in files(ql):
        for r in files(rl):
            ani = ref.pair(sk(q), sk(r), 1024)[2]
            if ani >= 700000:
                f.write("%%s\\t%%s\\t%%.4f\\t%%d\\t%%d\\n" %% (q, r, ani / 1e4, 1, 1))
"""


def text_tree(root):
    return {k: (None if v is None else v.decode()) for k, v in ref.snapshot(root).items()}


def main(scripts):
    spec = importlib.util.spec_from_file_location("extract_cluster", os.path.join(scripts, "extract_cluster_V4.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["extract_cluster"] = mod       # its worker processes pickle the instance by the module's name
    spec.loader.exec_module(mod)
    clusters = cases.golden_clusters()
    ids = [i for c in clusters for i, _ in c]
    seqs = [s for c in clusters for _, s in c]
    cluster_of = [k for k, c in enumerate(clusters) for _ in c]
    reps = [cluster_of.index(k) for k in range(len(clusters))]
    clstr = cluster_ref.clstr_text(ids, seqs, cluster_of, reps, [len(s) for s in seqs])
    flags = cases.GOLDEN_FLAGS
    out = {"meta": dict(flags, s=1024, floor=0.7)}
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        open("in.fa", "w").write("".join("%s\n%s\n" % (i, s) for i, s in zip(ids, seqs)))
        open("in.clstr", "w").write(clstr)
        mod.Extract_Cluster(Sequence_file="in.fa", Cluster_file="in.clstr", Outfile="cluster.txt", Identity_file="cluster.identities.txt",
                            Seq_number=500, Cluster_fa="Clusters_fa", nproc=1).run()
        os.remove("in.fa"), os.remove("in.clstr"), os.remove("cluster.identities.txt")
        snap = ref.snapshot(td)
        out["input"] = text_tree(td)
        os.makedirs(os.path.join(td, "bin"))
        tool = os.path.join(td, "bin", "fastANI")
        open(tool, "w").write(STAND_IN % (sys.executable, TESTS))
        os.chmod(tool, os.stat(tool).st_mode | stat.S_IXUSR)
        env = dict(os.environ, PATH=os.path.join(td, "bin") + os.pathsep + os.environ["PATH"])
        for mode in ("T", "F"):
            with tempfile.TemporaryDirectory() as run:
                ref.restore(run, snap)
                subprocess.run([sys.executable, os.path.join(scripts, "merge_cluster_by_ANI_V3.py"), "-i", "cluster.txt", "-p", "1", "-t", str(flags["t"]),
                                "-d", mode, "-a", str(flags["a"]), "-o", "history.txt"], cwd=run, env=env, check=True, stdout=subprocess.DEVNULL)
                out[mode] = text_tree(run)
                print("-d", mode, "history:", out[mode]["history.txt"].replace("\n", " | "))
        os.chdir(HERE)
    for mode in ("T", "F"):                    # the golden case holds no chain: no merged cluster also receives
        lines = [x.split("\t") for x in out[mode]["history.txt"].splitlines()]
        assert lines and not {r for r, _ in lines} & {s for _, s in lines}
    with open(os.path.join(HERE, "ani_small.json.gz"), "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
        g.write(json.dumps(out, sort_keys=True).encode())
    print(len(ids), "records,", len(clusters), "clusters,", os.path.getsize(os.path.join(HERE, "ani_small.json.gz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
