"""Plain restatement of the star-alignment rule of include/mprime_star.h — the yardstick of tests/test_star_gpu.py, checked itself
by tests/test_star.py.  Built on the anchored-alignment yardstick (anchor_ref.align, anchor_ref.anchor_of); nothing here knows how the
device schedules its work.  A helper, not a test."""
from __future__ import annotations

from anchor_ref import ACGT, align, anchor_of

MAX_BAND = 255
MAX_LEN = 32767
META_FIELDS = ("score", "d0", "n_match", "n_ins", "n_del", "first_col", "last_col", "status", "band")


def clean(record):
    """A record as the rule sees it: upper case, `-` and `.` removed."""
    r = record.decode("latin-1") if isinstance(record, (bytes, bytearray)) else str(record)
    return r.upper().replace("-", "").replace(".", "")


def align_escalating(q, anchor, band, **kw):
    """Steps 1 and 2: the anchored rule at W, again at min(2 W, 255) while the path touches the band's edge or there is none; the vote is
    taken once.  Returns (result of the last attempt, its W)."""
    n = len(anchor)
    col = list(range(n))
    res = align(q, anchor, col, n, band=band, **kw)
    W = band
    while (res["status"] & 2) and W < MAX_BAND:            # (status 3 has bit 1 set)
        W = min(2 * W, MAX_BAND)
        res = align(q, anchor, col, n, band=W, d0=res["d0"], **kw)
    return res, W


def runs_of(res):
    """{slot: (first query base, length)} of the inserted runs of a path, and [(query base, anchor position)] of its pairs."""
    runs, pairs = {}, []
    i, j = 0, res["anchor_start"]
    for op in res["ops"]:
        if op == "M":
            pairs.append((i, j))
            i, j = i + 1, j + 1
        elif op == "D":
            j += 1
        else:
            if j in runs:
                assert runs[j][0] + runs[j][1] == i, "two runs in one slot"
                runs[j] = (runs[j][0], runs[j][1] + 1)
            else:
                runs[j] = (i, 1)
            i += 1
    return runs, pairs


def star_round(records, anchor, band=32, match=5, mismatch=4, gap_open=10, gap_extend=2, min_identity_permille=500):
    """One round: dict(rows, meta, ins, width, acol, placed, counts).  rows[q] is None for an unplaced record."""
    n = len(anchor)
    kw = dict(match=match, mismatch=mismatch, gap_open=gap_open, gap_extend=gap_extend, min_identity_permille=min_identity_permille)
    results = [align_escalating(q, anchor, band, **kw) for q in records]
    meta = [dict(score=r["score"], d0=r["d0"], n_match=r["n_match"], n_ins=r["n_ins"], n_del=r["n_del"], first_col=r["first_col"],
                 last_col=r["last_col"], status=r["status"], band=W) for r, W in results]
    placed = [not (r["status"] & 1) and r["status"] != 3 for r, _ in results]
    paths = [runs_of(r) if ok else None for (r, _), ok in zip(results, placed)]
    ins = [0] * (n + 1)
    for path in paths:
        if path:
            for j, (_, length) in path[0].items():
                ins[j] = max(ins[j], length)
    acol, total = [], 0
    for j in range(n + 1):
        total += ins[j]
        acol.append(j + total)                          # (acol[n] = L': slot n owns the last ins[n] columns)
    width = n + total
    rows = []
    for q, path in zip(records, paths):
        if path is None:
            rows.append(None)
            continue
        runs, pairs = path
        row = ["-"] * width
        for i, j in pairs:
            row[acol[j]] = q[i]
        for j, (start, length) in runs.items():
            first = acol[j] - ins[j]
            if start == 0:                              # the run before the first M / D: right-justified
                first += ins[j] - length
            row[first:first + length] = q[start:start + length]
        rows.append("".join(row))
    kept = [r for r in rows if r is not None]
    counts = []
    for c in range(width):
        letters = [r[c] for r in kept]
        counts.append([letters.count(b) for b in ACGT] + [sum(1 for x in letters if x not in ACGT and x != "-"), letters.count("-")])
    return dict(rows=rows, meta=meta, ins=ins, width=width, acol=acol, placed=placed, counts=counts)


def centre_of(records):
    """Index of round 0's anchor: the longest record, the earliest among equals."""
    return max(range(len(records)), key=lambda q: (len(records[q]), -q))


def star(records, rounds=2, **kw):
    """The whole rule on cleaned records: dict(rounds=[round dicts], anchors=[anchor of every round run]); the output is rounds[-1]."""
    assert 1 <= rounds <= 8 and len(records) >= 1
    for q in records:
        if not 1 <= len(q) <= MAX_LEN:
            raise ValueError(f"record of {len(q)} bases (1..{MAX_LEN})")
    anchor = records[centre_of(records)]
    out = dict(rounds=[], anchors=[])
    for k in range(rounds):
        res = star_round(records, anchor, **kw)
        out["rounds"].append(res)
        out["anchors"].append(anchor)
        if k + 1 == rounds:
            break
        kept = [r for r in res["rows"] if r is not None]
        if not kept:
            raise ValueError("no record placed")
        nxt = anchor_of(kept)[0]
        if not 1 <= len(nxt) <= MAX_LEN:
            raise ValueError(f"consensus of {len(nxt)} letters (1..{MAX_LEN})")
        if nxt == anchor:
            break
        anchor = nxt
    return out
