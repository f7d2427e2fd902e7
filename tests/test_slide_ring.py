"""The sliding evaluation's ring of reference-mismatch words is addressed by OFFSETS that the band routine (csrc/slidecore.hpp) moves on by
one slot per window — the slot it writes and one per strict position it reads — instead of slot numbers recomputed per read.  What can go
wrong with that is a wrap: the shapes here are the smallest at which every offset wraps several times in a band (3 k windows and more), at
which a band ends before the first wrap (1, 2, k - 1 windows; an odd number of iterations), the warm-up leaves no / one column to the main loop
(k - 1 even / odd), a window in the middle of a band has no chains (its iteration must still move every offset), and the strict sets take
every way the routine reads them: none, one position per side at either end (shared, or each side its own), two and three per side all
distinct, the default `-c 2,3,-1` sets — the shapes read position by distinct position —, three per side all shared and two against one
(the masked reads), four on a side (the per-position form).

The same list runs twice: on the CPU through tools/slide_emul.cpp's `ring` mode (the band routine one lane at a time against brute force, every
ring access bounds-checked) and on the GPU (MP_EVAL_SLIDE=1) against the oracle, candidate by candidate."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO


def strict_sets(k):
    return {
        "none": ((), ()),
        "first": ((0,), (0,)),
        "last": ((k - 1,), (k - 1,)),
        "default": ((2, 3), (2, k - 3, k - 2)),
        "one_each": ((0,), (k - 1,)),
        "two_each": ((0, 1), (k - 2, k - 1)),
        "two_one": ((1, 2), (k - 1,)),
        "distinct3": ((0, 2, 3), (1, k - 2, k - 1)),
        "shared3": ((1, 3, k - 2), (1, 3, k - 2)),
        "four": ((0, 1, 2, 3), (2,)),
    }


def cases():
    """(k, v, rows, band, gw, strict set, MP_SLIDE_STRICT)"""
    out = []
    # every k with every band length, the default sets: k - 1 = 17, 30, 5 (odd: one warm-up column left to the main loop), 18, 8 (even: none)
    for i, k in enumerate((18, 19, 31, 6, 9)):
        for band in (1, 2, k - 1, 3 * k + 2):
            out.append((k, (i + band) % 4, 40, band, 2, "default", 1))
    # every strict set: wrapping bands and bands that end before the first wrap
    for k in (18, 31):
        for name in strict_sets(k):
            if name != "default":
                out.append((k, 1, 40, 3 * k + 2, 2, name, 1))
                out.append((k, 2, 40, k - 1, 1, name, 1))
    # v = 0 .. 3 (the default sets at k = 18 in a wrapping band; v = 1 is above)
    for v in (0, 2, 3):
        out.append((18, v, 40, 3 * 18, 2, "default", 1))
    # rows: one partly live wave; a second wave with one live lane (32 x 2 x 64 + 1 at two words per lane); two row slices with dead waves in
    # the second (a slice = 256 lanes x gw words x 32 rows) — at 1, 2 and 4 words per lane
    for gw in (1, 2, 4):
        for rows in (40, 32 * gw * 64 + 1, 256 * gw * 32 + 32 * gw * 64 + 1):
            out.append((18, 1, rows, 3 * 18 + 1, gw, "default", 1))
    # the per-position form as a cross-check of the same addressing
    out.append((18, 1, 40, 3 * 18, 2, "default", 0))
    out.append((19, 2, 4097, 18, 2, "shared3", 0))
    return sorted(set(out))


CASES = cases()


def case_id(c):
    k, v, rows, band, gw, name, strict = c
    return f"k{k}-v{v}-rows{rows}-band{band}-gw{gw}-{name}-strict{strict}"


def mask_of(positions):
    return sum(1 << p for p in positions)


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slide_ring") / "slide_emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", os.path.join(REPO, "tools", "slide_emul.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_band_routine_on_the_cpu(emul, case):
    k, v, rows, band, gw, name, strict = case
    sf, sr = strict_sets(k)[name]
    rows = min(rows, 2100)                                  # the emulation runs one lane at a time: a lane is a lane at any row count
    out = subprocess.run([emul, "ring", str(k), str(v), str(rows), str(band), str(gw), "%x" % mask_of(sf), "%x" % mask_of(sr), str(strict)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert b"equal to brute force" in out.stdout


def ring_chains(rng, root, W, k, strict):
    """Refinement chains off the consensus, most degenerate member first (the items that slide), most steps widening a strict position; every
    seventh window has none."""
    cw, codes = [], []
    for w in range(W):
        if w % 7 == 3:
            continue
        for _ in range(int(rng.integers(1, 3))):
            cur = root[w: w + k].copy()
            chain = [cur.copy()]
            for _ in range(int(rng.integers(1, 8))):
                at_strict = len(strict) > 0 and rng.random() < 0.6
                cur[int(rng.choice(strict)) if at_strict else int(rng.integers(0, k))] |= np.uint8(1 << rng.integers(0, 4))
                chain.append(cur.copy())
            chain.reverse()
            cw += [w] * len(chain)
            codes += chain
    return np.asarray(cw, np.int32), np.asarray(codes, np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_sliding_kernel_matches_oracle(hip_lib, oracle_lib, monkeypatch, case):
    import torch  # noqa: F401  (before the HIP library is used: the first HIP runtime loaded serves the process)
    from test_hip_parity import both, fuzz_msa
    k, v, rows, band, gw, name, strict = case
    sf, sr = strict_sets(k)[name]
    p0 = 2
    W = max(band + 9, 30)                                   # more than one band, the last one shorter
    L = W + k + p0 + 3
    data, off, _ = fuzz_msa(9000 + 31 * k + rows + v, rows, L, ragged=False, p_gap=0.03, p_iupac=0.002)
    rng = np.random.default_rng(rows * 13 + 5 * k + v + band)
    root = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, size=L)]
    cw, codes = ring_chains(rng, root, W, k, sorted(set(sf) | set(sr)))
    hip, ora = both(hip_lib, oracle_lib, data, off)
    for c in (hip, ora):
        c.build_windows(p0, W, k, v)
    want = ora.eval_candidates(cw, codes, mask_of(sf), mask_of(sr))
    monkeypatch.setenv("MP_EVAL_SLIDE", "1")
    monkeypatch.setenv("MP_SLIDE_BAND", str(band))
    monkeypatch.setenv("MP_SLIDE_GW", str(gw))
    if not strict:
        monkeypatch.setenv("MP_SLIDE_STRICT", "0")
    got = hip.eval_candidates(cw, codes, mask_of(sf), mask_of(sr))
    info = hip.eval_plan_info()
    hip.close()
    ora.close()
    # the sliding kernel answered, not the first-pass kernels in its place: every chain is a simple item off the consensus
    assert info["sliding_items"] >= 0.9 * info["chain_items"] > 0, info
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{bad.size} candidates differ, the first: candidate {bad[0]} (window {cw[bad[0]]}): {got[bad[0]]} against {want[bad[0]]}"
