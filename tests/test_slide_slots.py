"""The walk of the sliding evaluation (csrc/slidecore.hpp, slide_item) ends at an item's last member slot (SLIDE_WALK_EXIT): the slots behind it
are neither updated nor counted, and their words of the workgroup's table hold whatever the registers held.  What can go wrong with that: an
exit one slot early or late, a member that reports a slot the walk did not write, the count of a reverse side that shares its word with a
slot that was not walked, planes and counts of a LONG item showing through in the short one that follows it in the other register set or, two
items on, in the same one.

The chains are made by rule, the same one as tools/slide_emul.cpp's `slots` mode (make_slots_case, which says why each part is there): 43
windows, window 21 without chains; chain A of 1 + w % 8 member slots in window w and, in every third window, chain B of 8 - w % 8; every event
the loss of a base beyond the root of its column, the last one at a strict position (forward only / reverse only / both / none, by turns); by
turns one event per step, an eventless step (two equal neighbours) and two events in one step (a slot nobody reports).  Where chain A or B would
be the root k-mer alone next to the other one's eight slots, the library reads that candidate as one more member of the other chain (nested
runs are maximal): those windows hold one chain of eight slots whose last step has no event.  Every number of slots 1 .. 8 is carried by at
least four of the 52 items.

The CPU test runs the band routine one lane at a time against brute force (`slots` mode: every slot a member reports must be one the walk
wrote, every number of slots must have slid) — for these chains the plan builder leaves out none at k = 18 and at most three at k = 6 (ties
of the reference vote in the few columns that a single window covers).  The GPU test (MP_EVAL_SLIDE=1) compares with the oracle candidate by
candidate — on rows drawn around the rule's own root, so that the counts are real: non-zero in nearly every window and different from slot to
slot (asserted; 4097-row cases for every number of levels, where every event moves a count) — and asks for the ring test's bound, sliding_items >= 0.9 x chain_items, and — from the CPU run — for fewer items left out than
the smallest class has, so that no number of slots can hide among them."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

W, P0, SKIP = 43, 2, 21


def strict_sets(k):
    return {"none": ((), ()), "default": ((2, 3), (2, k - 3, k - 2)), "four": ((0, 1, 2, 3), (2,))}


def cases():
    """(k, v, rows, band, gw, strict set, MP_SLIDE_STRICT)"""
    out = []
    for k in (18, 6):
        for v in (0, 1, 2, 3):                                  # the thermometer updates of the walk differ by the number of levels
            for band in (8, 100):                               # bands of 8 windows; one band for all
                out.append((k, v, 40, band, 2, "default", 1))
        out.append((k, 1, 40, 8, 2, "none", 1))
        out.append((k, 2, 40, 100, 2, "none", 1))
        out.append((k, 1, 40, 8, 2, "four", 0))                 # the per-position strict form
        out.append((k, 3, 40, 100, 2, "four", 0))
    for gw in (1, 2, 4):                                        # one partly live wave; a second wave with one live lane
        for rows in (40, 32 * gw * 64 + 1):
            out.append((18, 1, rows, 8, gw, "default", 1))
            out.append((6, 2, rows, 100, gw, "default", 1))
    # 40 rows leave few rows per count; every number of levels and both other strict forms once more where every event moves a count
    for v in (0, 2, 3):
        out.append((18, v, 4097, 8, 2, "default", 1))
    out.append((18, 2, 4097, 8, 2, "none", 1))
    out.append((18, 1, 4097, 100, 2, "four", 0))
    return sorted(set(out))


CASES = cases()


def case_id(c):
    k, v, rows, band, gw, name, strict = c
    return f"k{k}-v{v}-rows{rows}-band{band}-gw{gw}-{name}-strict{strict}"


def mask_of(positions):
    return sum(1 << p for p in positions)


def root_base(c):
    return (5 * c + c // 3) % 4


def slots_chain(w, chain, n_slots, form, k, sf, sr):
    """The members of one chain (symbol sets per position), most degenerate first: tools/slide_emul.cpp slots_chain."""
    n_ev = n_slots - 1
    root = [root_base(P0 + w + j) for j in range(k)]
    by_class = (0, sf & ~sr, sr & ~sf, sf & sr)[(w + chain) % 4]
    last_pos = (by_class & -by_class).bit_length() - 1 if by_class else -1
    last = (last_pos, (root[last_pos] + 1 + w % 3) % 4 if last_pos >= 0 else 0)
    ev, i = [], 0
    while len(ev) < n_ev:
        if len(ev) == n_ev - 1 and last_pos >= 0:
            ev.append(last)
            break
        pos = (7 * w + 5 * i) % k
        pb = (pos, (root[pos] + 1 + (i // k + pos + w) % 3) % 4)
        if pb != last and pb not in ev:
            ev.append(pb)
        i += 1
    steps = [[e] for e in range(n_ev)]
    if form == 1 and 1 <= n_ev <= 6:
        steps.insert((n_ev + 1) // 2, [])
    if form in (2, 3) and n_ev >= 2:
        steps[0].append(1)
        del steps[1]
    if form == 3:
        steps.append([])
    top = np.array([1 << b for b in root], np.uint8)
    for pos, base in ev:
        top[pos] |= 1 << base
    members = [top]
    for st in steps:
        m = members[-1].copy()
        for e in st:
            m[ev[e][0]] &= ~np.uint8(1 << ev[e][1])
        members.append(m)
    return members


def slots_chains(k, sf, sr):
    """(candidate windows, candidate codes, number of chains, items per number of member slots)"""
    cw, codes, n_chains, by_slots = [], [], 0, [0] * 9

    def add(w, chain, n_slots, form):
        nonlocal n_chains
        mem = slots_chain(w, chain, n_slots, form, k, sf, sr)
        cw.extend([w] * len(mem))
        codes.extend(mem)
        n_chains += 1
        by_slots[n_slots] += 1

    for w in range(W):
        if w == SKIP:
            continue
        sa, sb, two = 1 + w % 8, 8 - w % 8, w % 3 == 0
        if two and 1 in (sa, sb):
            add(w, 0, 8, 3)
            continue
        add(w, 0, sa, (w // 8) % 3)
        if two:
            add(w, 1, sb, (w // 8 + 1) % 3)
    return np.asarray(cw, np.int32), np.asarray(codes, np.uint8), n_chains, by_slots


def test_every_number_of_slots_is_carried():
    """What the bounds of the GPU test rest on: 52 chains, each number of member slots on at least four of them."""
    for k in (18, 6):
        for sf, sr in strict_sets(k).values():
            cw, codes, n_chains, by_slots = slots_chains(k, mask_of(sf), mask_of(sr))
            assert n_chains == 52 and min(by_slots[1:]) >= 4 and sum(by_slots) == 52, by_slots
            assert len(cw) == len(codes) and codes.shape[1] == k and (codes != 0).all()


def slots_msa(seed, n, L):
    """n rows around the RULE's root (the chains' root is the column consensus, so the counts are real): a tenth of the bases replaced by
    another one — what the chains' events accept —, a few gaps and IUPAC codes, an all-gap row and two long end gaps."""
    rng = np.random.default_rng(seed)
    base = np.array([root_base(c) for c in range(L)])[None, :].repeat(n, axis=0)
    sub = rng.random((n, L)) < 0.10
    base = np.where(sub, (base + rng.integers(1, 4, size=(n, L))) % 4, base)
    rows = np.frombuffer(b"ACGT", np.uint8)[base]
    rows = np.where(rng.random((n, L)) < 0.01, np.uint8(ord("-")), rows)
    junk = np.frombuffer(b"RYMKSWHBVDNn", np.uint8)
    rows = np.where(rng.random((n, L)) < 0.002, junk[rng.integers(0, len(junk), (n, L))], rows).astype(np.uint8)
    if n > 6:
        rows[3, :] = ord("-")
        rows[4, : L // 2] = ord("-")
        rows[5, L // 3:] = ord("-")
    return rows.reshape(-1), np.arange(n + 1, dtype=np.int64) * L


def counts_are_real(want, cw, codes, v):
    """What the comparison with the oracle is worth: (share of the windows with chains whose candidates have a non-zero perfect / forward /
    reverse count, share of the chains of two slots and more whose first and last member differ in a count, share of the steps with an event
    across which a count changes)."""
    wins = np.unique(cw)
    shares = [np.mean([(want[cw == w][:, c] != 0).any() for w in wins]) for c in range(3)]
    ends, steps = [], []
    starts = np.flatnonzero(np.r_[True, (cw[1:] != cw[:-1]) | ((codes[1:] & ~codes[:-1]) != 0).any(axis=1)])     # a chain ends where a member is not within the one before
    for b, e in zip(starts, np.r_[starts[1:], len(cw)]):
        if (codes[b] != codes[e - 1]).any():
            ends.append((want[b] != want[e - 1]).any())
        steps += [(want[i] != want[i + 1]).any() for i in range(b, e - 1) if (codes[i] != codes[i + 1]).any()]
    return shares, float(np.mean(ends)), float(np.mean(steps))


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slide_slots") / "slide_emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", os.path.join(REPO, "tools", "slide_emul.cpp"), "-o", exe])
    return exe


def test_chains_are_the_emulation_s(emul):
    """The rule is written twice, here and in tools/slide_emul.cpp: candidate by candidate the same windows and symbol sets."""
    for k in (18, 6):
        for sf, sr in strict_sets(k).values():
            out = subprocess.run([emul, "chains", str(k), "%x" % mask_of(sf), "%x" % mask_of(sr)], stdout=subprocess.PIPE, check=True, timeout=60)
            theirs = np.array([[int(x) for x in line.split()] for line in out.stdout.decode().splitlines()])
            cw, codes, _, _ = slots_chains(k, mask_of(sf), mask_of(sr))
            assert theirs.shape == (len(cw), k + 1) and (theirs[:, 0] == cw).all() and (theirs[:, 1:] == codes).all(), (k, sf, sr)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_walk_on_the_cpu(emul, case):
    k, v, rows, band, gw, name, strict = case
    sf, sr = strict_sets(k)[name]
    rows = min(rows, 2100)                                  # the emulation runs one lane at a time: a lane is a lane at any row count
    out = subprocess.run([emul, "slots", str(k), str(v), str(rows), str(band), str(gw), "%x" % mask_of(sf), "%x" % mask_of(sr), str(strict)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    text = out.stdout.decode()
    assert "equal to brute force" in text
    m = re.search(r"\((\d+) items slid, (\d+) left out\); items by member slots 1\.\.8:((?: \d+){8})", text)
    assert m, text
    slid, left, hist = int(m.group(1)), int(m.group(2)), [int(x) for x in m.group(3).split()]
    assert min(hist) > 0 and sum(hist) == slid, text        # every number of member slots slid
    assert left <= 2 * 3 and slid + left == 2 * 52, text    # (two alignments per run) what the GPU test's bound on items left out rests on


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_sliding_kernel_matches_oracle(hip_lib, oracle_lib, monkeypatch, case):
    import torch  # noqa: F401  (before the HIP library is used: the first HIP runtime loaded serves the process)
    from test_hip_parity import both
    k, v, rows, band, gw, name, strict = case
    sf, sr = strict_sets(k)[name]
    L = W + k + P0 + 3
    data, off = slots_msa(7000 + 31 * k + rows + v, rows, L)          # (not fuzz_msa: its rows have a root of their own, far from the chains')
    cw, codes, n_chains, by_slots = slots_chains(k, mask_of(sf), mask_of(sr))
    hip, ora = both(hip_lib, oracle_lib, data, off)
    for c in (hip, ora):
        c.build_windows(P0, W, k, v)
    want = ora.eval_candidates(cw, codes, mask_of(sf), mask_of(sr))
    # The comparison is worth something only where the counts are not all zero and move along a chain — a hole that still holds the count of
    # the item before, a plane of that item ORed in, an exit one slot early must CHANGE a number.  A row matches a position with
    # 0.99 x 0.9 and carries a given other base with 0.033: at k = 18 an eighth of the rows is perfect (4.6 of the ~37 that are no end gap:
    # a window without one in 100), and an event changes the perfect count of 40 rows with 1 - exp(-37 x 0.033 x 0.14) = 0.16 (v = 0, the
    # least), a chain's ends with ~0.5; from 2049 rows on every event moves ~8 rows.  Bounds: two to three standard deviations below that.
    shares, ends, steps = counts_are_real(want, cw, codes, v)
    print(case_id(case), "windows with non-zero counts", shares, "chains whose ends differ", ends, "event steps that change a count", steps)
    assert shares[0] >= 0.9 and (v == 0 or min(shares[1:]) >= 0.9), shares
    assert (ends >= 0.95 and steps >= 0.95) if rows >= 2049 else (ends >= 0.3 and steps >= 0.1), (ends, steps)
    monkeypatch.setenv("MP_EVAL_SLIDE", "1")
    monkeypatch.setenv("MP_SLIDE_BAND", str(band))
    monkeypatch.setenv("MP_SLIDE_GW", str(gw))
    if not strict:
        monkeypatch.setenv("MP_SLIDE_STRICT", "0")
    got = hip.eval_candidates(cw, codes, mask_of(sf), mask_of(sr))
    info = hip.eval_plan_info()
    hip.close()
    ora.close()
    print(case_id(case), info)
    # the library found the chains as they were made, and the sliding kernel answered, not the first-pass kernels in its place
    assert info["chain_items"] == n_chains, info
    assert info["sliding_items"] >= 0.9 * info["chain_items"] > 0, info
    assert info["chain_items"] - info["sliding_items"] < min(by_slots[1:]), info
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} candidates differ, the first: candidate {bad[0]} (window {cw[bad[0]]}): {got[bad[0]]} against {want[bad[0]]}"
