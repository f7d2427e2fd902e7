"""Inputs of the star-alignment tests (tests/test_star.py checks what they are meant to provoke on the yardstick alone,
tests/test_star_gpu.py compares the device with the yardstick on them).  A helper, not a test.  Every group is a list of records as
they stand in a FASTA (any case, `-` and `.` allowed), a parameter set and a number of rounds."""
import random

import star_ref as ref
from anchor_cases import planted_indel, rand_seq, substitute


def group(name, records, rounds=2, band=32, match=5, mismatch=4, gap_open=10, gap_extend=2, min_identity_permille=500, **extra):
    return dict(name=name, records=list(records), rounds=rounds,
                params=dict(band=band, match=match, mismatch=mismatch, gap_open=gap_open, gap_extend=gap_extend,
                            min_identity_permille=min_identity_permille), **extra)


def other_than(rng, *letters):
    return rng.choice([b for b in "ACGT" if b not in letters])


def insert_run(rng, left, right, g):
    """g bases to insert between `left` and `right` so that no shifted gap scores the same: the run neither ends in `left` nor starts
    with `right`."""
    x = [other_than(rng, right)] + [rng.choice("ACGT") for _ in range(g - 1)]
    x[-1] = other_than(rng, left, right) if g == 1 else other_than(rng, left)
    return "".join(x)


def plant(rng, anc, n_sub, indels, quiet=12, apart=10):
    """A child of `anc`: `indels` gaps of 1..8 bases (no two closer than `apart`, none within `quiet` of an end, each placed so that no
    shifted gap scores the same) and n_sub substitutions at least 6 bases away from every gap and outside the quiet ends.  Returns
    (child, homology): homology[i] = the ancestor position of child base i, None for an inserted base."""
    n = len(anc)
    while True:
        sites = sorted(rng.sample(range(quiet + 8, n - quiet - 8), indels))
        if all(b - a >= apart + 8 for a, b in zip(sites, sites[1:])):
            break
    edits = {}
    for p in sites:
        g = rng.randint(1, 8)
        if rng.random() < 0.5:                           # delete anc[p:p+g]: neither neighbour repeats across the gap
            while anc[p - 1] == anc[p + g - 1] or anc[p] == anc[p + g]:
                p += 1
            edits[p] = ("del", g)
        else:                                            # insert before anc[p]: the run's ends differ from both neighbours
            edits[p] = ("ins", insert_run(rng, anc[p - 1], anc[p], g))
    blocked = set()
    for p, (kind, what) in edits.items():
        blocked.update(range(p - 6, p + (what if kind == "del" else 0) + 6))
    free = [p for p in range(quiet, n - quiet) if p not in blocked]
    subs = {p: other_than(rng, anc[p]) for p in rng.sample(free, n_sub)}
    child, hom, p = [], [], 0
    while p < n:
        if p in edits:
            kind, what = edits[p]
            if kind == "del":
                p += what
                continue
            child += list(what)
            hom += [None] * len(what)
            edits = {k: v for k, v in edits.items() if k != p}
            continue
        child.append(subs.get(p, anc[p]))
        hom.append(p)
        p += 1
    return "".join(child), hom


def planted_family(seed=1, n=150, children=12):
    """The ancestor (the longest record, so round 0's anchor) and children that differ by substitutions and 1..3 planted gaps."""
    rng = random.Random(seed)
    anc = rand_seq(rng, n)
    records, homs = [anc], [list(range(n))]
    while len(records) <= children:
        child, hom = plant(rng, anc, rng.randint(0, 5), rng.randint(1, 3))
        if len(child) < n:
            records.append(child)
            homs.append(hom)
    return group(f"family{seed}", records, homology=homs)


def hand_groups():
    rng = random.Random(17)
    c = rand_seq(rng, 100)                               # n + 1 = 101: not a multiple of 16
    out = []
    # slot 0 and slot n; the leading runs of 3 and of 1 base share slot 0, the shorter one right-justified
    out.append(group("slot0-slotn", [c, "TTT" + c[:70], "G" + c[:60], c[20:] + "GGA", c[35:] + other_than(rng, c[-1])]))
    # two records inserting 2 and 5 bases in slot 40
    x2, x5 = insert_run(rng, c[39], c[40], 2), insert_run(rng, c[39], c[40], 5)
    out.append(group("same-slot", [c, c[:40] + x2 + c[40:95], c[5:40] + x5 + c[40:90]], runs=(x2, x5)))
    # a leading run (right-justified) and an interior run (left-justified) in one record; another record widens both slots
    x3, x5 = insert_run(rng, c[29], c[30], 3), insert_run(rng, c[29], c[30], 5)
    lead = other_than(rng, c[0])
    out.append(group("lead-and-interior", [c, 2 * lead + c[:30] + x3 + c[30:70], "AC" + 2 * lead + c[:30] + x5 + c[30:80]], runs=(lead, x3, x5)))
    # I directly followed by D: with a mismatch dearer than two one-base gaps a substitution becomes an insertion and a deletion
    s = list(c[:90])
    s[45] = other_than(rng, s[45], c[44], c[46])
    out.append(group("ins-then-del", [c, "".join(s)], mismatch=30))
    # an unplaced record of another composition must not widen any slot
    ct = rand_seq(rng, 100, "CT")
    out.append(group("unplaced", [ct, ct[:50] + "CTT" + ct[50:95], rand_seq(rng, 60, "AG"), substitute(rng, ct[10:], 3)]))
    # gap_open = 0: opening costs what extending does, so every inserted base of a run "opens" it anew — the runs of 2, 5 and 3 (leading)
    # bases and the 3 bases of slot n must each stay one run of their slot
    # (runs of one letter that none of the two anchor bases on either side is: with free opening a mixed run would split to gain a match)
    far = other_than(rng, *c[38:42])
    x2, x5 = 2 * far, 5 * far
    out.append(group("gap-open-0", [c, c[:40] + x2 + c[40:95], c[5:40] + x5 + c[40:90], "TTT" + c[:70], c[20:] + "GGA"], gap_open=0, runs=(x2, x5)))
    out.append(group("single", [c[:57]]))
    out.append(group("identical", [c] * 5, rounds=3))
    # `-`, `.` and lower case inside records
    out.append(group("gapped-input", [c, c[:30].lower() + "--" + c[30:60] + ".." + c[62:], "-" + c[3:50] + "-", c[:20] + "ga" + c[20:80]]))
    return out


def drift_groups():
    """anchor_cases.planted_indel: one gap of g bases that only a band of at least g admits; the anchor is padded so that it is the longest
    record.  g = 40: touched at W = 32, clear at 64 (the inserted run of 40 crosses a writer lane's 16 bytes).  g = 300: still touched at 255."""
    rng = random.Random(23)
    out = []
    for kind in ("ins", "del"):
        anchor, query = planted_indel(32, 40, kind)
        out.append(group(f"drift-64-{kind}", [anchor + rand_seq(rng, 30, "CGT"), query, anchor[:90]]))
    # the same construction with a gap of 300 and a run of A long enough for the 268 bases the narrowest band leaves over: inserting
    # one more base of the gap (2) is cheaper than pairing it with an A (4), so the best path runs along the band's edge at every W
    head = rand_seq(rng, 159) + "G"
    query = substitute(rng, head, 3, 5, 150) + rand_seq(rng, 299, "CGT") + "C" + "A" * 30
    anchor = head + "A" * 320 + rand_seq(rng, 20, "CGT")
    out.append(group("drift-255", [anchor, query, anchor[10:200]], rounds=1))
    return out


def consensus_groups():
    rng = random.Random(29)
    anc = rand_seq(rng, 110)
    # the centre carries a private insertion and private substitutions: the consensus of round 0 drops them
    centre = substitute(rng, anc[:50], 2, 12, 40) + "GATTA" + anc[50:]
    kids = [substitute(rng, anc[a:b], 2, 14, 60) for a, b in ((0, 110), (0, 110), (0, 110), (0, 110), (2, 108), (1, 109))]
    out = [group("consensus-moves", [centre] + kids, rounds=3, ancestor=anc)]
    # the centre is the ancestor, every child differs in its own places: the consensus is the centre and the loop stops after one round
    kids = []
    for k in range(6):
        q = substitute(rng, anc, 3, 12 + 14 * k, 24 + 14 * k)
        p = 15 + 13 * k
        kids.append(q[:p] + q[p + 2:] if k % 2 else q[:p] + "TG" + q[p:105])
    out.append(group("consensus-stays", [anc] + kids, rounds=3))
    return out


def batch_group(n_records=200, seed=31):
    """Short records from the 200-base anchor of planted_indel(32, 40, "del"); every tenth is its query, whose path touches the band at
    W = 32 (it is aligned again at 64)."""
    rng = random.Random(seed)
    anc, drifting = planted_indel(32, 40, "del")
    records = [anc]
    while len(records) < n_records:
        if len(records) % 10 == 3:
            records.append(drifting)
            continue
        m = rng.randint(50, 90)
        a0 = rng.randint(0, 130 - m)
        q = list(substitute(rng, anc[a0:a0 + m], rng.randint(0, 3)))
        if rng.random() < 0.5:
            p, g = rng.randint(8, m - 8), rng.randint(1, 4)
            q[p:p] = list(rand_seq(rng, g))
        records.append("".join(q))
    return group("batch200", records)


def all_groups():
    return hand_groups() + drift_groups() + consensus_groups() + [planted_family(1), planted_family(2, n=97, children=8)]


def cleaned(g):
    return [ref.clean(r) for r in g["records"]]


def yardstick(g):
    return ref.star(cleaned(g), rounds=g["rounds"], **g["params"])
