"""Plain restatement of the both-strand rule (include/mprime_anchor.h: ORIENTATION, include/mprime_star.h, include/mprime_cluster.h:
BOTH STRANDS) — the yardstick of tests/test_strand_gpu.py, checked itself by tests/test_strand.py.  Built on the forward-only yardsticks
(anchor_ref, star_ref, cluster_ref), which it calls on the oriented record and never changes; nothing here knows how the device schedules
its work.  A helper, not a test."""
from __future__ import annotations

import anchor_ref as aref
import cluster_ref as cref
import star_ref as sref

REVERSED = 8                                     # status bit 3: the reverse complement of the input record
COMPLEMENT = {"A": "T", "T": "A", "U": "A", "C": "G", "G": "C", "R": "Y", "Y": "R", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H",
              "H": "D"}                          # S, W, N and every other byte: unchanged


def upper(s):
    """a-z to A-Z, every other byte as it is (what the device does to a letter)."""
    s = s.decode("latin-1") if isinstance(s, (bytes, bytearray)) else str(s)
    return "".join(chr(ord(ch) - 32) if "a" <= ch <= "z" else ch for ch in s)


def rc(s):
    """The upper-cased record reversed, each letter complemented."""
    return "".join(COMPLEMENT.get(ch, ch) for ch in reversed(upper(s)))


def rc_codes(s):
    """rc as the clustering code store sees it: only A, C, G, T (codes 0 .. 3) are complemented, every other letter keeps its code —
    so `U`, which rc turns into A, stays a letter that matches nothing."""
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}.get(ch, ch) for ch in reversed(upper(s)))


def best_vote(q, a):
    """(votes, diagonal) of the best diagonal of votes(q, a), (0, None) without a vote."""
    v = aref.votes(upper(q), a)
    if not v:
        return 0, None
    d = min(v, key=lambda d: (-v[d], abs(d), d))
    return v[d], d


def orient(q, a):
    """(the record as it is aligned, turned): rc(q) iff its best diagonal has strictly more votes than q's."""
    turned = best_vote(rc(q), a)[0] > best_vote(q, a)[0]
    return (rc(q) if turned else q), turned


# ---- anchored alignment ---------------------------------------------------------------------------------------------------------------
def align(query, anchor, col, width, **kw):
    """anchor_ref.align of the oriented query; status bit 3 and `reversed` say whether it was turned."""
    q, turned = orient(query, anchor)
    out = aref.align(q, anchor, col, width, **kw)
    out["reversed"] = turned
    if turned:
        out["status"] |= REVERSED
    return out


# ---- star alignment -------------------------------------------------------------------------------------------------------------------
def star(records, rounds=2, **kw):
    """star_ref.star with every round voting both strands of the records as they are held: dict(rounds, anchors, parity) — parity[k][q]
    after round k, against the input; a round's meta status carries it as bit 3 and its rows are those of the held records."""
    assert 1 <= rounds <= 8 and len(records) >= 1
    held = [sref.clean(r) for r in records]
    parity = [False] * len(held)
    anchor = held[sref.centre_of(held)]                  # the longest record in its given orientation
    out = dict(rounds=[], anchors=[], parity=[])
    for k in range(rounds):
        for q in range(len(held)):
            held[q], turned = orient(held[q], anchor)
            parity[q] ^= turned
        res = sref.star_round(held, anchor, **kw)
        for q, mt in enumerate(res["meta"]):
            if parity[q]:
                mt["status"] |= REVERSED
        out["rounds"].append(res)
        out["anchors"].append(anchor)
        out["parity"].append(list(parity))
        if k + 1 == rounds:
            break
        kept = [r for r in res["rows"] if r is not None]
        if not kept:
            raise ValueError("no record placed")
        nxt = aref.anchor_of(kept)[0]
        if nxt == anchor:
            break
        anchor = nxt
    return out


def oriented_id(ident, turned):
    return ">_R_" + ident[1:] if turned else ident


def anchor_files(seed_ids, seed_rows, ids, queries, results, strands, keep_seed=True):
    """(OUT, OUT.anchor.tsv, OUT.unaligned.fa) of scripts/anchor_msa.py from the yardstick's results."""
    fa = "".join("%s\n%s\n" % (i, r) for i, r in zip(seed_ids, seed_rows)) if keep_seed else ""
    tsv = "id\tstatus\tscore\td0\tn_match\tn_ins\tn_del\tfirst_col\tlast_col" + ("\tstrand\n" if strands else "\n")
    un = ""
    for i, q, r in zip(ids, queries, results):
        turned = bool(r["status"] & REVERSED)
        if r["status"] & 1:
            un += "%s\n%s\n" % (i, q)
        else:
            fa += "%s\n%s\n" % (oriented_id(i, turned), r["row"])
        tsv += "\t".join(str(x) for x in (i, r["status"], r["score"], r["d0"], r["n_match"], r["n_ins"], r["n_del"], r["first_col"], r["last_col"]))
        tsv += ("\t-\n" if turned else "\t+\n") if strands else "\n"
    return fa, tsv, un


def star_files(ids, records, res, strands):
    """(OUT, OUT.star.tsv, OUT.unaligned.fa) of scripts/run_mafft.py from star()'s (or star_ref.star's) result."""
    last = res["rounds"][-1]
    fa, un = "", ""
    tsv = "id\tstatus\tband\tscore\td0\tn_match\tn_ins\tn_del" + ("\tstrand\n" if strands else "\n")
    for i, rec, row, mt in zip(ids, records, last["rows"], last["meta"]):
        turned = bool(mt["status"] & REVERSED)
        if mt["status"] & 1:
            un += "%s\n%s\n" % (i, rec)
        else:
            fa += "%s\n%s\n" % (oriented_id(i, turned), row)
        tsv += "\t".join(str(x) for x in (i, mt["status"], mt["band"], mt["score"], mt["d0"], mt["n_match"], mt["n_ins"], mt["n_del"]))
        tsv += ("\t-\n" if turned else "\t+\n") if strands else "\n"
    for k, (rnd, anchor) in enumerate(zip(res["rounds"], res["anchors"])):
        tsv += "# round {}: n {} width {} placed {} band_warnings {}\n".format(k, len(anchor), rnd["width"], sum(rnd["placed"]),
                                                                             sum(1 for mt in rnd["meta"] if mt["status"] & 2))
    return fa, tsv, un


# ---- clustering -----------------------------------------------------------------------------------------------------------------------
def pair(s, r, strand, **kw):
    """cluster_ref.pair with rc of the query where strand = 1; the anchor is always the sequence as given."""
    return cref.pair(rc_codes(s) if strand else upper(s), upper(r), **kw)


def similar_pm(s, r, memo=None, **kw):
    """(n_match, strand) under similar+-: the forward test first, the reverse test only when it fails; None when neither holds."""
    nm = cref.similar(upper(s), upper(r), memo=memo, **kw)
    if nm is not None:
        return nm, 0
    nm = cref.similar(rc_codes(s), upper(r), memo=memo, **kw)
    return None if nm is None else (nm, 1)


def cluster(seqs, memo=None, **kw):
    """Sequential greedy under both strands: (cluster_of [n], rep_of_cluster [n_clusters], n_match_of [n], strand_of [n])."""
    seqs = [upper(s) for s in seqs]
    order = sorted(range(len(seqs)), key=lambda i: (-len(seqs[i]), i))
    cluster_of, n_match_of, strand_of, reps = [-1] * len(seqs), [0] * len(seqs), [0] * len(seqs), []
    for i in order:
        for k, r in enumerate(reps):
            hit = similar_pm(seqs[i], seqs[r], memo=memo, **kw)
            if hit is not None:
                cluster_of[i], n_match_of[i], strand_of[i] = k, hit[0], hit[1]
                break
        else:
            cluster_of[i], n_match_of[i] = len(reps), len(seqs[i])
            reps.append(i)
    return cluster_of, reps, n_match_of, strand_of


def clstr_text(ids, seqs, cluster_of, reps, n_match_of, strand_of):
    """The .clstr file of a both-strand run: member lines `at +/dd.dd%` / `at -/dd.dd%`, as cd-hit-est prints them."""
    members = [[] for _ in reps]
    for i, k in enumerate(cluster_of):
        members[k].append(i)
    lines = []
    for k, mem in enumerate(members):
        lines.append(">Cluster %d" % k)
        for x, i in enumerate(mem):
            tail = "*" if i == reps[k] else "at %s/%s" % ("-" if strand_of[i] else "+", cref.identity_text(n_match_of[i], len(seqs[i])))
            lines.append("%d\t%daa, %s... %s" % (x, len(seqs[i]), ids[i], tail))
    return "\n".join(lines) + "\n"
