"""Plain restatement of the clustering rule of include/mprime_cluster.h — the yardstick of tests/test_cluster_gpu.py, checked itself
by tests/test_cluster.py.  Sort, sequential greedy, similar() on the votes and the alignment of tests/anchor_ref.py with the
representative as the anchor (col = range(n)); nothing here knows of blocks, rounds or batches.  A helper, not a test."""
from __future__ import annotations

import anchor_ref as ref

NO_SCORE = ref.NO_SCORE
DEFAULTS = dict(band=32, identity_permille=800, min_votes=1, match=5, mismatch=4, gap_open=10, gap_extend=2)


def read_fasta(text):
    """[(id, sequence)]: the id is the header's first token ('>' included), the sequence upper-cased."""
    if isinstance(text, (bytes, bytearray)):
        text = text.decode("latin-1")
    out = []
    for line in text.splitlines():
        line = line.strip()
        if line.startswith(">"):
            out.append([line.split()[0], []])
        elif line and out:
            out[-1][1].append(line.upper())
    return [(i, "".join(s)) for i, s in out]


def pair(s, r, band=32, identity_permille=800, min_votes=1, match=5, mismatch=4, gap_open=10, gap_extend=2):
    """dict(votes, d0, score, n_match, status) of query s against anchor r."""
    s, r = s.upper(), r.upper()
    v = ref.votes(s, r)
    d0 = ref.seed_diagonal(s, r)
    votes = v.get(d0, 0)
    if votes < min_votes:
        return dict(votes=votes, d0=d0, score=NO_SCORE, n_match=0, status=5)
    a = ref.align(s, r, list(range(len(r))), len(r), band=band, match=match, mismatch=mismatch, gap_open=gap_open, gap_extend=gap_extend,
                  min_identity_permille=identity_permille, d0=d0)
    return dict(votes=votes, d0=d0, score=a["score"], n_match=a["n_match"], status=a["status"])


def similar(s, r, memo=None, identity_permille=800, **kw):
    """n_match when s is similar to r, else None.  `memo` (a dict) keeps the pair records between calls that differ in
    identity_permille only: the alignment does not depend on it, the decision is taken here."""
    p = memo.get((s, r)) if memo is not None else None
    if p is None:
        p = pair(s, r, identity_permille=identity_permille, **kw)
        if memo is not None:
            memo[(s, r)] = p
    return p["n_match"] if p["score"] != NO_SCORE and p["n_match"] * 1000 >= identity_permille * len(s) else None


def cluster(seqs, **kw):
    """Sequential greedy over `seqs` (strings): (cluster_of [n], rep_of_cluster [n_clusters], n_match_of [n])."""
    seqs = [s.upper() for s in seqs]
    order = sorted(range(len(seqs)), key=lambda i: (-len(seqs[i]), i))
    cluster_of, n_match_of, reps = [-1] * len(seqs), [0] * len(seqs), []
    for i in order:
        for k, r in enumerate(reps):
            nm = similar(seqs[i], seqs[r], **kw)
            if nm is not None:
                cluster_of[i], n_match_of[i] = k, nm
                break
        else:
            cluster_of[i], n_match_of[i] = len(reps), len(seqs[i])
            reps.append(i)
    return cluster_of, reps, n_match_of


def identity_text(n_match, m):
    v = (n_match * 10000 + m // 2) // m
    return "%d.%02d%%" % (v // 100, v % 100)


def clstr_text(ids, seqs, cluster_of, reps, n_match_of):
    """The .clstr file: members in input order inside a cluster, numbered from 0."""
    members = [[] for _ in reps]
    for i, k in enumerate(cluster_of):
        members[k].append(i)
    lines = []
    for k, mem in enumerate(members):
        lines.append(">Cluster %d" % k)
        for x, i in enumerate(mem):
            tail = "*" if i == reps[k] else "at " + identity_text(n_match_of[i], len(seqs[i]))
            lines.append("%d\t%daa, %s... %s" % (x, len(seqs[i]), ids[i], tail))
    return "\n".join(lines) + "\n"


def rep_fasta(ids, seqs, reps):
    return "".join("%s\n%s\n" % (ids[i], seqs[i].upper()) for i in reps)


def parse_clstr(text):
    """Written from the format lines alone: [[(number, length, id, '*' or 'dd.dd%')]] per cluster."""
    out = []
    for line in text.splitlines():
        if line.startswith(">Cluster "):
            assert int(line[len(">Cluster "):]) == len(out)
            out.append([])
            continue
        num, rest = line.split("\t")
        length, rest = rest.split("aa, ", 1)
        ident, tail = rest.split("... ", 1)
        assert ident.startswith(">")
        if tail != "*":
            assert tail.startswith("at ") and tail.endswith("%")
            tail = tail[3:]
        out[-1].append((int(num), int(length), ident, tail))
    return out
