"""Plain restatement of the anchored-alignment rule of include/mprime_anchor.h — the yardstick of tests/test_anchor_gpu.py, checked
itself by tests/test_anchor.py.  Written from the rule, row by row, with true -inf for cells that do not exist; nothing here knows how
the device schedules its work.  A helper, not a test."""
from __future__ import annotations

NINF = float("-inf")
ACGT = "ACGT"
WORD = 12
NO_SCORE = -(1 << 31)
DEFAULTS = dict(match=5, mismatch=4, gap_open=10, gap_extend=2)


def anchor_of(seed_rows):
    """(anchor, col) of a seed alignment given as equal-length strings / bytes."""
    rows = [r.decode("latin-1") if isinstance(r, (bytes, bytearray)) else str(r) for r in seed_rows]
    rows = [r.upper() for r in rows]
    n_rows, width = len(rows), len(rows[0])
    assert all(len(r) == width for r in rows)
    anchor, col = [], []
    for c in range(width):
        letters = [r[c] for r in rows if r[c] != "-"]
        if 2 * len(letters) <= n_rows:
            continue
        best, best_n = "N", 0
        for b in ACGT:
            k = letters.count(b)
            if k > best_n:
                best, best_n = b, k
        anchor.append(best)
        col.append(c)
    return "".join(anchor), col


def pair_score(x, y, match, mismatch):
    if x in ACGT and y in ACGT:
        return match if x == y else -mismatch
    return 0


def votes(q, a):
    """{diagonal: votes} of the 12-letter words q and a share."""
    where = {}
    for j in range(len(a) - WORD + 1):
        w = a[j:j + WORD]
        if all(ch in ACGT for ch in w):
            where.setdefault(w, []).append(j)
    out = {}
    for i in range(len(q) - WORD + 1):
        for j in where.get(q[i:i + WORD], ()):
            out[j - i] = out.get(j - i, 0) + 1
    return out


def seed_diagonal(q, a):
    v = votes(q, a)
    if not v:
        return min(max(0, -len(q)), len(a))
    return min(v, key=lambda d: (-v[d], abs(d), d))


def align(query, anchor, col, width, band=32, match=5, mismatch=4, gap_open=10, gap_extend=2, min_identity_permille=500, d0=None):
    """One query against the anchor: dict(row, score, d0, n_match, n_ins, n_del, first_col, last_col, status, ops)."""
    q = query.decode("latin-1") if isinstance(query, (bytes, bytearray)) else str(query)
    q = q.upper()
    a = anchor
    m, n = len(q), len(a)
    if d0 is None:
        d0 = seed_diagonal(q, a)
    lo, hi = d0 - band, d0 + band
    oe = gap_open + gap_extend

    # full (m + 1) x (n + 1) tables, -inf wherever a cell does not exist (outside the band included)
    H = [[NINF] * (n + 1) for _ in range(m + 1)]
    E = [[NINF] * (n + 1) for _ in range(m + 1)]
    F = [[NINF] * (n + 1) for _ in range(m + 1)]
    for j in range(max(0, lo), min(n, hi) + 1):
        H[0][j] = 0
    for i in range(1, m + 1):
        Hi, Ei, Fi, Hu, Fu, qi = H[i], E[i], F[i], H[i - 1], F[i - 1], q[i - 1]
        for j in range(max(0, i + lo), min(n, i + hi) + 1):
            if j >= 1:
                e = max(Hi[j - 1] - oe, Ei[j - 1] - gap_extend)
                g = Hu[j - 1] + pair_score(qi, a[j - 1], match, mismatch)
            else:
                e = g = NINF
            f = max(Hu[j] - oe, Fu[j] - gap_extend)
            Ei[j], Fi[j], Hi[j] = e, f, max(g, e, f)
    ends = range(max(0, m + lo), min(n, m + hi) + 1)
    best = max((H[m][j] for j in ends), default=NINF)
    out = dict(d0=d0, row="-" * width, ops="", n_match=0, n_ins=0, n_del=0, first_col=-1, last_col=-1, anchor_start=-1, anchor_end=-1)
    if best == NINF:
        out.update(score=NO_SCORE, status=3)
        return out
    j = min(j for j in ends if H[m][j] == best)
    i, state, ops, row, touch = m, "H", [], ["-"] * width, False
    out["anchor_end"] = j                      # anchor positions [anchor_start, anchor_end) lie opposite the ops
    pairs = []
    while True:
        touch = touch or (j - i) in (lo, hi)
        if state == "H":
            if i == 0:
                break
            g = H[i - 1][j - 1] + pair_score(q[i - 1], a[j - 1], match, mismatch) if j >= 1 else NINF
            if H[i][j] == g:
                ops.append("M")
                pairs.append((i - 1, j - 1))
                i, j = i - 1, j - 1
            elif H[i][j] == E[i][j]:
                state = "E"
            else:
                state = "F"
        elif state == "E":                      # (j >= 1: E(i, 0) is -inf and never chosen)
            ops.append("D")
            if E[i][j] == H[i][j - 1] - oe:
                state = "H"
            j -= 1
        else:
            ops.append("I")
            if F[i][j] == H[i - 1][j] - oe:
                state = "H"
            i -= 1
    out["anchor_start"] = j
    ops.reverse()
    pairs.reverse()
    for qi, aj in pairs:
        row[col[aj]] = q[qi]
    n_match = sum(1 for qi, aj in pairs if q[qi] in ACGT and q[qi] == a[aj])
    status = (1 if n_match * 1000 < min_identity_permille * m else 0) | (2 if touch else 0)
    out.update(score=int(best), row="".join(row), ops="".join(ops), n_match=n_match, n_ins=ops.count("I"), n_del=ops.count("D"),
               first_col=col[pairs[0][1]] if pairs else -1, last_col=col[pairs[-1][1]] if pairs else -1, status=status)
    return out


def align_all(seed_rows, queries, **kw):
    anchor, col = anchor_of(seed_rows)
    width = len(seed_rows[0])
    return [align(q, anchor, col, width, **kw) for q in queries]
