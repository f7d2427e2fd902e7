"""Inputs that take the star alignment's assembly kernels and its batching past one tile (csrc/star.hip: the flag scan, the chunked
escalation list, the profile, scan, map, write and count kernels, the launch planning at the length limit).  tests/test_star.py checks on
the yardstick alone that every group provokes what it is for, tests/test_star_edges.py compares the device with the yardstick on them.
A helper, not a test.  Every group is one round: records, the anchor the round is run against, and the parameters."""
import functools
import random

import numpy as np

import star_ref as ref
from anchor_cases import planted_indel, rand_seq, substitute
from star_cases import cleaned, group, insert_run, other_than

LEVELS = {4: 0, 8: 1, 16: 2, 32: 3, 64: 4, 128: 5, 255: 6}       # escalations behind a final band, from band = 4 (and from 32)


def edge_group(name, records, anchor, **kw):
    return group(name, records, rounds=1, anchor=anchor, **kw)


_truth = {}


def yardstick_round(g):
    """The yardstick's one round of a group against its anchor, computed once per process and never changed."""
    if g["name"] not in _truth:
        _truth[g["name"]] = ref.star_round(cleaned(g), g["anchor"], **g["params"])
    return _truth[g["name"]]


# ---- A: many tiny records ------------------------------------------------------------------------------------------------------------
TINY_SIZES = (256, 257, 1024, 1025, 2049)
TINY_BAND_OF_RUN = {3: 4, 4: 8, 5: 8, 8: 16, 9: 16, 16: 32, 17: 32, 20: 32}      # where a record with one inserted run ends, from band = 4
TINY_STRANGERS = (7, 255, 256, 1023, 1024, 2047)           # unplaced: a profile (256) and a count (1024) workgroup start and end on one


def tiny_plan(N):
    """Which records of a batch of N carry a run that the band of 4 does not admit, fixed by position and not only by rate:
    dict(per, strangers, flagged, full, quiet) — `per` records per thread of the flag scan, `full` a thread's slice flagged throughout,
    `quiet` 200 slices in a row without a flagged record (batches of at least 1024 records)."""
    per = (N + 1023) // 1024
    strangers = {q for q in TINY_STRANGERS if q < N}
    quiet, threads = range(0), [5, N // per // 3, 2 * (N // per) // 3]
    if N >= 1024:
        t0 = 260
        while any(per * t0 <= q < per * (t0 + 200) for q in strangers):
            t0 += 1
        quiet = range(per * t0, per * (t0 + 200))
        threads = [5, t0 - 3, t0 + 203]
    for k, t in enumerate(threads):                      # (not where a stranger stands)
        while {per * t - 1, per * t, per * t + 1} & strangers:
            t -= 1
        threads[k] = t
    full = range(per * 20, per * 21)
    flagged = {1, 2, 3, 4, N - 3, N - 2, N - 1} | set(full)
    for t in threads:
        flagged |= {per * t - 1, per * t, per * t + 1}
    assert all(0 < q < N for q in flagged) and not flagged & set(quiet)
    return dict(per=per, strangers=strangers, flagged=flagged - strangers, full=full, quiet=quiet, threads=threads)


@functools.lru_cache(maxsize=None)
def many_tiny(N, seed=41):
    """A 48-base anchor (record 0) and N - 1 records of 20..40 of its bases, band = 4.  The planned records and about one in seven of the
    others carry one inserted run of 4..20 bases (they end at band 8, 16 or 32), one in twenty a run of 3 (it stays at 4).  Every such
    record, and every A / G stranger, is drawn until the yardstick gives it the band (or the rejection) it is there for."""
    rng = random.Random(seed)
    anc = rand_seq(rng, 48)
    plan = tiny_plan(N)
    long_runs = [g for g in TINY_BAND_OF_RUN if g > 3]
    records, runs = [anc], {}

    def drawn(make, wanted):
        """A band narrower than the run does not always touch its edge: behind the flank that lost the vote a path of mismatches may
        score as well as one along the edge.  Draw until the yardstick says what the record is meant to provoke."""
        while True:
            q = make()
            if wanted(*ref.align_escalating(q, anc, 4)):
                return q

    def with_run(g):
        m = rng.randint(24, 40)                          # both flanks hold a 12-mer
        s = rng.randint(0, 48 - m)
        p = rng.randint(s + 12, s + m - 12)
        return anc[s:p] + insert_run(rng, anc[p - 1], anc[p], g) + anc[p:s + m]

    for q in range(1, N):
        if q in plan["strangers"]:
            records.append(drawn(lambda: rand_seq(rng, rng.randint(20, 40), "AG"), lambda res, W: res["status"] & 1))
            continue
        draw = rng.random()
        g = 0
        if q in plan["flagged"] or (q not in plan["quiet"] and draw < 1 / 7):
            g = long_runs[(q + len(runs)) % len(long_runs)]
        elif draw > 0.95:
            g = 3
        if g:
            records.append(drawn(lambda: with_run(g), lambda res, W: W == TINY_BAND_OF_RUN[g] and res["status"] == 0 and res["n_ins"] == g))
            runs[q] = g
        else:
            m = rng.randint(20, 40)
            s = rng.randint(0, 48 - m)
            records.append(anc[s:s + m])
    return edge_group(f"tiny{N}", records, anc, band=4, plan=plan, runs=runs)


# ---- B: rows narrower than a writer lane's 16 bytes -------------------------------------------------------------------------------------
def one_letter():
    """L' = 1: 1024 records A, one C (a mismatch, so unplaced: the second count workgroup starts on it), five more A."""
    return edge_group("one-letter", ["A"] * 1024 + ["C"] + ["A"] * 5, "A", band=4)


def short_rows():
    return edge_group("width7", ["ACGTA", "A", "AC", "ACG", "CGTA", "TTTTT", "GGACG", "GTA", "TA", "ACGT", "G"], "ACGTA", band=4)


def width15(seed=43):
    """A 13-base anchor and a leading run of two: rows of 15 bytes, an unplaced record between placed ones, a tail of the row buffer that
    is no multiple of 16."""
    rng = random.Random(seed)
    anc = rand_seq(rng, 13)
    lead = other_than(rng, anc[0])
    rare = min("ACGT", key=anc.count)
    records = [anc, 2 * lead + anc[:12], anc[1:], rare * 9, anc[:12], lead + anc, anc[1:13], rare * 12, anc]
    return edge_group("width15", records, anc, band=4)


# ---- C: long anchors -----------------------------------------------------------------------------------------------------------------
LONG_SIZES = (1023, 1024, 2047, 2048, 2100)


def long_plan(n, seed):
    """{slot: run length}: slot 0, slot n, the slots on either side of 1023 / 1024 and 2047 / 2048, and the first and the last slot of
    six slices of the column scan (per = ceil((n + 1) / 1024) slots to a thread; twelve single slots where per = 1)."""
    rng = random.Random(seed)
    per = (n + 1 + 1023) // 1024
    slots = {0, n} | {j for j in (1023, 1024, 2047, 2048) if j <= n}
    fractions = (0.03, 0.15, 0.3, 0.62, 0.75, 0.9) + ((0.1, 0.2, 0.4, 0.55, 0.7, 0.85) if per == 1 else ())
    threads = [int(f * (n + 1) / per) for f in fractions]
    for t in threads:
        slots |= {per * t, per * t + per - 1}
    return {j: rng.randint(1, 6) for j in sorted(slots)}, per, threads


def long_anchor(name, n, plan, seed):
    """The anchor (record 0) and records of 200..300 of its bases; between them they carry the planned runs, one or two to a record."""
    rng = random.Random(seed)
    anc = rand_seq(rng, n)
    held = []                                            # the slots of every record, ascending
    for j in sorted(plan):
        home = next((h for h in held if len(h) < 2 and 25 <= j - h[-1] <= 150 and h[0] != 0 and j != n), None)
        if home is None:
            held.append([j])
        else:
            home.append(j)
    records = [anc]
    for q, h in enumerate(held):
        spare = 200 + 23 * (q % 5) - (h[-1] - h[0])      # bases beside the runs: neighbours differ in ceil(m / 8)
        s, e = h[0] - spare // 2, h[-1] + spare - spare // 2
        if h[0] == 0 or s < 0:
            s, e = 0, h[-1] + spare
        if h[-1] == n or e > n:
            s, e = h[0] - spare, n
        parts, at = [], s
        for j in h:
            parts += [anc[at:j], insert_run(rng, anc[j - 1] if j else anc[0], anc[j] if j < n else anc[n - 1], plan[j])]
            at = j
        records.append("".join(parts) + anc[at:e])
    return edge_group(name, records, anc, plan=plan, held=held)


def long_groups():
    out = []
    for n in LONG_SIZES:
        plan, per, threads = long_plan(n, 50 + n)
        out.append(dict(long_anchor(f"long{n}", n, plan, 60 + n), per=per, threads=threads))
    # n = 1000 and 24 / 25 inserted columns: L' = 1024 and 1025
    for extra in (0, 1):
        plan = {0: 3, 130: 3, 300: 3, 470: 3, 512: 3, 700: 3, 890: 3 + extra, 1000: 3}
        out.append(long_anchor(f"width{1024 + extra}", 1000, plan, 70))
    return out


# ---- D: a flagged list longer than the traceback buffer -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chunked_list(seed=47):
    """band = 32, one batch of 45 records in which every record but the anchor is flagged.  The anchor is that of planted_indel(32, 40,
    "del") followed by a second construction of the same kind with a gap of 70 and a run of 60 A.  Two records in three are the first
    construction's query (its head with substitutions of their own, the tail of A trimmed): touched at 32, clear at 64.  Every third is
    the second one's (50 A behind the head: taking W of the 70 bases along the band's edge pays at W = 32 and at 64): clear at 128."""
    rng = random.Random(seed)
    base, _ = planted_indel(32, 40, "del")
    head = base[:100]
    head2 = rand_seq(rng, 99) + "G"
    anchor = base + head2 + rand_seq(rng, 69, "CGT") + "C" + "A" * 60 + rand_seq(rng, 20, "CGT")
    records, kinds = [anchor], [0]
    while len(records) < 45:
        kind = 2 if len(records) % 3 == 2 else 1
        if kind == 1:
            q = substitute(rng, head, rng.randint(2, 3), 5, 90) + "A" * (30 - rng.randint(0, 9))       # (under 20 A the edge no longer pays at 32)
        else:
            cut = rng.randint(0, 12)
            q = substitute(rng, head2[cut:], 2, 5, 80) + "A" * 50
        if (len(q) + 7) // 8 != (len(records[-1]) + 7) // 8 and q not in records:
            records.append(q)
            kinds.append(kind)
    return edge_group("chunked", records, anchor, band=32, kinds=kinds)


def flagged_words(g, truth, first, last, diagonals):
    """Traceback words of the records [first, last) that the yardstick aligns again beyond the first band, at `diagonals` per lane:
    (rows rounded up to eight) x 64 lanes x diagonals."""
    return sum((len(r) + 7) // 8 * 64 * diagonals
               for r, m in zip(cleaned(g)[first:last], truth["meta"][first:last]) if m["band"] > g["params"]["band"])


# ---- E: the length limit ---------------------------------------------------------------------------------------------------------------
def limit_case(length, seed=9):
    """Three records at `length` and what the rule gives for them, from the planted homology alone: a random anchor; a copy with a
    substitution every 53 bases (none within 60 of an end or within 100 of the inserted run: the diagonal path is optimal, a gap pair
    around a substitution would cost 24 to save 9); the fragment anchor[100:a] + run + anchor[a:b] with a run of three bases that neither
    ends in anchor[a - 1] nor starts with anchor[a].  The longer part anchor[100:a] wins the vote: d0 = 100."""
    rng = random.Random(seed)
    gen = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    a_arr = letters[gen.integers(0, 4, length)]
    a, b = (55 * length) // 100, length - 150
    pos = np.arange(60, length - 60, 53)
    pos = pos[np.abs(pos - a) >= 100]
    c_arr = a_arr.copy()
    c_arr[pos] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(letters, a_arr[pos])]
    anchor, copy = a_arr.tobytes().decode(), c_arr.tobytes().decode()
    run = insert_run(rng, anchor[a - 1], anchor[a], 3)
    fragment = anchor[100:a] + run + anchor[a:b]
    k = len(pos)
    rows = [anchor[:a] + "---" + anchor[a:], copy[:a] + "---" + copy[a:], "-" * 100 + fragment + "-" * (length - b)]
    arr = np.array([np.frombuffer(r.encode(), np.uint8) for r in rows])
    per_letter = [(arr == ord(x)).sum(axis=0) for x in "ACGT-"]
    counts = np.stack(per_letter[:4] + [3 - sum(per_letter), per_letter[4]], axis=1)
    fields = ref.META_FIELDS
    meta = [dict(zip(fields, (5 * length, 0, length, 0, 0, 0, length - 1, 0, 32))),
            dict(zip(fields, (5 * (length - k) - 4 * k, 0, length - k, 0, 0, 0, length - 1, 0, 32))),
            dict(zip(fields, (5 * (b - 100) - (10 + 2 * 3), 100, b - 100, 3, 0, 100, b - 1, 0, 32)))]
    ins = [0] * (length + 1)
    ins[a] = 3
    star = dict(rows=rows, meta=meta, ins=ins, width=length + 3, counts=counts.tolist(), placed=[True] * 3)
    # anchored alignment of the copy and the fragment on identity columns: the inserted bases have no column
    anchored = [dict({f: meta[1][f] for f in fields[:8]}, row=copy, ops="M" * length),
                dict({f: meta[2][f] for f in fields[:8]}, row="-" * 100 + anchor[100:b] + "-" * (length - b),
                     ops="M" * (a - 100) + "III" + "M" * (b - a))]
    return dict(anchor=anchor, records=[anchor, copy, fragment], a=a, b=b, substitutions=k, star=star, anchored=anchored)
