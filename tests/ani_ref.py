"""Plain restatement of the rule of include/mprime_ani.h — the yardstick of tests/test_ani_gpu.py, checked itself by tests/test_ani.py:
words and their hash, the bottom-s sketch, a pair's (w, u, ani_ppm), the table, two groups' (n_rep, sum_ppm), the merge decision over
a cluster list, history.txt and the file operations on a Clusters_fa tree.  Sets, sorted lists and loops; nothing here knows of tiles,
blocks or batches.  A helper, not a test."""
from __future__ import annotations

import math
import os
import shutil

WORD = 12
PPM = 1000000
_M = 0xFFFFFFFF


def fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M
    h ^= h >> 16
    return h


def words(seq):
    """The set of 24-bit values of the words of seq (first letter most significant)."""
    codes = ["ACGT".find(chr(b & 0xDF)) for b in seq.encode("latin-1")]
    out = set()
    for i in range(len(codes) - WORD + 1):
        w = codes[i:i + WORD]
        if min(w) >= 0:
            v = 0
            for cd in w:
                v = v * 4 + cd
            out.add(v)
    return out


def sketch(seq, s=1024):
    return sorted(fmix32(v) for v in words(seq))[:s]


def table():
    tab = [0]
    for q in range(1, 1025):
        j = q / 1024.0
        tab.append(max(0, int(math.floor(1e6 * (1.0 + math.log(2.0 * j / (1.0 + j)) / 12.0) + 0.5))))
    return tab


TAB = table()


def pair(a, b, s):
    """(w, u, ani_ppm) of two sketches at size s."""
    lasts = [x[-1] for x in (a, b) if len(x) == s]
    c = min(lasts) if lasts else None
    sa = {x for x in a if c is None or x <= c}
    sb = {x for x in b if c is None or x <= c}
    w = len(sa & sb)
    u = len(sa) + len(sb) - w
    return w, u, TAB[(w * 1024) // u if u else 0]


def groups(p_sketches, r_sketches, s, report_ppm):
    """(n_rep, sum_ppm) over all (p, r)."""
    n_rep = total = 0
    for a in p_sketches:
        for b in r_sketches:
            ani = pair(a, b, s)[2]
            if ani >= report_ppm:
                n_rep += 1
                total += ani
    return n_rep, total


# ---- the decision ------------------------------------------------------------------------------------------------------------------------
def parse_clusters(text):
    """[(name, size)] by size descending, ties in file order; a repeated name keeps its first place and its last size."""
    d = {}
    for line in text.splitlines(True):
        if not line.startswith("#"):
            f = line.strip().split("\t")
            d[f[0]] = int(f[1])
    return sorted(d.items(), key=lambda x: -x[1])


def work_dir(cluster_file):
    return cluster_file.rstrip("cluster.txt") + "Clusters_fa"


def visiting(clusters, t):
    """Positions of the processing clusters in visiting order."""
    if t == 1:
        return []
    return [p for p in range(len(clusters) - 1, -1, -1) if t == 0 or clusters[p][1] <= t]


def decide(clusters, t, ani_ppm, numbers):
    """[(ref position, sub position)] in visiting order; numbers(p, r) -> (n_rep, sum_ppm)."""
    out = []
    for p in visiting(clusters, t):
        for r in range(len(clusters)):
            if clusters[r][1] > clusters[p][1]:
                n_rep, total = numbers(p, r)
                if n_rep > 0 and total >= ani_ppm * n_rep:
                    out.append((r, p))
                    break
    return out


def merge_dict(clusters, wd, decided):
    """{ref id: [sub id]}: refs in order of first appearance, subs in visiting order."""
    ident = lambda x: "%s/%s_%d" % (wd, clusters[x][0], clusters[x][1])
    out = {}
    for r, p in decided:
        out.setdefault(ident(r), []).append(ident(p))
    return out


def history_text(md):
    return "".join("%s\t%s\n" % (k, m) for k, subs in md.items() for m in subs)


def apply(clusters, wd, md, drop):
    for name, size in clusters:
        shutil.rmtree("%s/%s_%d" % (wd, name, size), ignore_errors=True)
    if drop == "T":
        for ref, subs in md.items():
            for sub in subs:
                if sub not in md:
                    for ext in (".fa", ".tfa", ".txt"):
                        os.remove(sub + ext)
        return
    now = {}                                   # id -> the id its files carry now
    for ref in sorted(md, key=lambda x: int(x.rsplit("_", 1)[1])):       # receiving clusters by size ascending
        total = int(ref.rsplit("_", 1)[1])
        for sub in md[ref]:
            cur = now.get(sub, sub)
            total += int(cur.rsplit("_", 1)[1])
            for ext in (".fa", ".tfa", ".txt"):
                with open(ref + ext, "ab") as fo, open(cur + ext, "rb") as fi:
                    fo.write(fi.read())
                os.remove(cur + ext)
        final = "%s_%d" % (ref.rsplit("_", 1)[0], total)
        for ext in (".fa", ".tfa", ".txt"):
            os.rename(ref + ext, final + ext)
        now[ref] = final


# ---- trees -------------------------------------------------------------------------------------------------------------------------------
def read_fasta(path):
    out = []
    for line in open(path, encoding="latin-1"):
        line = line.strip()
        if line.startswith(">"):
            out.append([line.split()[0], ""])
        elif line and out:
            out[-1][1] += line
    return [(i, s) for i, s in out]


def tree_numbers(clusters, wd, s, report_ppm):
    """numbers(p, r) of decide() from the .tfa files of a tree, memoised."""
    sk, memo = {}, {}

    def sketches(x):
        if x not in sk:
            sk[x] = [sketch(seq, s) for _, seq in read_fasta("%s/%s_%d.tfa" % (wd, clusters[x][0], clusters[x][1]))]
        return sk[x]

    def numbers(p, r):
        if (p, r) not in memo:
            memo[(p, r)] = groups(sketches(p), sketches(r), s, report_ppm)
        return memo[(p, r)]
    return numbers


def snapshot(root):
    """{relative path: bytes, or None for a directory} of everything under root."""
    out = {}
    for d, dirs, files in os.walk(root):
        for x in dirs:
            out[os.path.relpath(os.path.join(d, x), root)] = None
        for x in files:
            out[os.path.relpath(os.path.join(d, x), root)] = open(os.path.join(d, x), "rb").read()
    return out


def restore(root, snap):
    for rel, data in sorted(snap.items()):
        path = os.path.join(root, rel)
        if data is None:
            os.makedirs(path, exist_ok=True)
        else:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as f:
                f.write(data)
