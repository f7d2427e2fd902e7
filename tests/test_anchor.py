"""The yardstick of anchored alignment (tests/anchor_ref.py, a plain restatement of the rule in include/mprime_anchor.h) checked on
its own, without a device: its score against an exhaustive enumeration of alignments, its outputs against each other, the anchor
construction (also the product's numpy form of it), the vote's tie-breaks, what the planted cases of tests/anchor_cases.py are meant
to provoke, and the command line's exit statuses."""
import itertools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import anchor_cases as cases
import anchor_ref as ref
from conftest import REPO

PARAM_SETS = (dict(match=5, mismatch=4, gap_open=10, gap_extend=2), dict(match=5, mismatch=4, gap_open=0, gap_extend=2),
              dict(match=2, mismatch=3, gap_open=1, gap_extend=0))


def _shapes(m, n):
    """Every alignment of m query bases to a stretch of n anchor positions that starts anywhere: (first anchor position, ops)."""
    def walk(i, j, ops):
        if i == m:
            yield "".join(ops)
        if i < m and j < n:
            yield from walk(i + 1, j + 1, ops + ["M"])
        if i < m:
            yield from walk(i + 1, j, ops + ["I"])
        if j < n:
            yield from walk(i, j + 1, ops + ["D"])
    for j0 in range(n + 1):
        for ops in walk(0, j0, []):
            yield j0, ops


def rescore(query, anchor, start, ops, match, mismatch, gap_open, gap_extend):
    """The ten-line scorer: pairs by the pair score, every maximal run of D or of I as one gap."""
    i, j, total, prev = 0, start, 0, ""
    for op in ops:
        if op == "M":
            total += ref.pair_score(query[i], anchor[j], match, mismatch)
            i, j = i + 1, j + 1
        else:
            total -= gap_extend + (gap_open if op != prev else 0)
            i, j = i + (op == "I"), j + (op == "D")
        prev = op
    assert i == len(query)
    return total


@pytest.mark.parametrize("par", PARAM_SETS, ids=lambda p: "m{match}x{mismatch}o{gap_open}e{gap_extend}".format(**p))
def test_score_is_the_maximum_over_all_alignments(par):
    """Every query / anchor pair over {A, C, G} with m <= 4, n <= 5, the band wide enough to hold everything.  The enumeration scores
    all letter pairs of one (m, n) at once: the pair score of query position i and anchor position j is a matrix over (query, anchor)."""
    for m in range(1, 5):
        queries = ["".join(t) for t in itertools.product("ACG", repeat=m)]
        qa = np.array([[ord(ch) for ch in q] for q in queries])
        for n in range(1, 6):
            anchors = ["".join(t) for t in itertools.product("ACG", repeat=n)]
            aa = np.array([[ord(ch) for ch in a] for a in anchors])
            pair = [[np.where(qa[:, i, None] == aa[None, :, j], par["match"], -par["mismatch"]) for j in range(n)] for i in range(m)]
            best = np.full((len(queries), len(anchors)), -10 ** 9)
            for start, ops in _shapes(m, n):
                i, j, prev = 0, start, ""
                total = np.zeros_like(best)
                for op in ops:
                    if op == "M":
                        total = total + pair[i][j]
                        i, j = i + 1, j + 1
                    else:
                        total = total - (par["gap_extend"] + (par["gap_open"] if op != prev else 0))
                        i, j = i + (op == "I"), j + (op == "D")
                    prev = op
                np.maximum(best, total, out=best)
            col = list(range(n))
            for qi, q in enumerate(queries):
                for ai, a in enumerate(anchors):
                    got = ref.align(q, a, col, n, band=m + n, d0=0, **par)
                    assert got["score"] == best[qi, ai], (q, a, par)


def test_outputs_agree_with_each_other():
    for g in cases.all_groups():
        p = g["params"]
        for q, r in zip(g["queries"], cases.yardstick(g)):
            if r["score"] == ref.NO_SCORE:
                assert r["status"] == 3 and r["ops"] == "" and set(r["row"]) == {"-"}
                continue
            ops, Q = r["ops"], q.upper()
            assert rescore(Q, g["anchor"], r["anchor_start"], ops, p["match"], p["mismatch"], p["gap_open"], p["gap_extend"]) == r["score"], g["name"]
            assert r["anchor_end"] - r["anchor_start"] == ops.count("M") + ops.count("D")
            kept, i = [], 0
            for op in ops:
                if op != "D":
                    if op == "M":
                        kept.append(Q[i])
                    i += 1
            assert r["row"].replace("-", "") == "".join(kept) and len(r["row"]) == g["width"], g["name"]
            assert (r["n_ins"], r["n_del"]) == (ops.count("I"), ops.count("D")) and len(ops) == len(q) + r["n_del"]
            i, j, n_match = 0, r["anchor_start"], 0
            for op in ops:
                n_match += op == "M" and Q[i] in "ACGT" and Q[i] == g["anchor"][j]
                i, j = i + (op != "D"), j + (op != "I")
            assert n_match == r["n_match"]
            if "M" in ops:
                assert r["row"][r["first_col"]] != "-" and r["row"][r["last_col"]] != "-"
                assert set(r["row"][: r["first_col"]] + r["row"][r["last_col"] + 1:]) <= {"-"}


def test_anchor_construction():
    from multiprime_amd.anchor import anchor_of
    seed = ["AC-TR-",
            "A--TY-",
            "CCGGN-",
            "C-G-RA"]
    # column 0: A and C tie -> A; 1 and 2: two of four rows is not strictly more than half; 3: T T G; 4: IUPAC only -> N; 5: one row
    assert ref.anchor_of(seed) == ("ATN", [0, 3, 4])
    assert ref.anchor_of(["ACGT", "ACGA", "A-GG"]) == ("ACGA", [0, 1, 2, 3])        # A, G, T once each in the last column: A
    assert ref.anchor_of(["TTGC", "GCCT", "CGTG"])[0] == "CCCC"                     # ties between C, G, T: C
    assert ref.anchor_of(["acgu-n"]) == ("ACGNN", [0, 1, 2, 3, 5])                  # one unaligned record, letters upper-cased
    rng = random.Random(2)
    for rows, width in ((1, 30), (2, 40), (5, 60), (16, 50)):
        seed = ["".join(rng.choice("ACGTacgtNRY---") for _ in range(width)) for _ in range(rows)]
        anchor, col = anchor_of([s.encode() for s in seed])
        assert (anchor.decode(), col.tolist()) == ref.anchor_of(seed)


def test_vote_ties_and_the_clamp():
    groups = {g["name"]: g for g in cases.tie_groups()}
    g = groups["vote-tie"]
    q_two, q_word, q_twice = g["queries"]
    assert ref.votes(q_two, g["anchor"]) == {-18: 1, 18: 1} and ref.seed_diagonal(q_two, g["anchor"]) == -18       # equal |d|: the smaller d
    assert ref.votes(q_word, g["anchor"]) == {4: 1, 40: 1} and ref.seed_diagonal(q_word, g["anchor"]) == 4        # the smaller |d|
    v = ref.votes(q_twice, g["anchor"])
    assert v[-8] == 2 and max(v.values()) == 2 and ref.seed_diagonal(q_twice, g["anchor"]) == -8                  # most votes beat the smaller |d|
    assert ref.seed_diagonal("ACGTACGTACGTAA", "ACGTACGTACGTACGTACGT") == 0                                       # most votes first: 3, 2, 1
    assert ref.votes("ACGTACGTACGTAA", "ACGTACGTACGTACGTACGT") == {0: 2, 4: 2, 8: 1}
    # no vote: a word with a letter outside A/C/G/T, a query shorter than a word, an empty anchor
    assert ref.seed_diagonal("ACGTNCGTACGTA", "ACGTACGTACGTACGT") == 0 and ref.seed_diagonal("ACGT", "ACGTACGTACGTACGT") == 0
    assert ref.seed_diagonal("ACGT", "") == 0
    for q, a in (("A" * 40, "A" * 13), ("ACGT" * 5, "ACGT" * 9)):
        assert -len(q) <= ref.seed_diagonal(q, a) <= len(a)


def test_planted_cases_provoke_what_they_are_meant_to():
    for g in cases.band_groups():
        W = g["params"]["band"]
        kind, gap = ("del", int(g["name"].split("del")[1])) if "del" in g["name"] else ("ins", int(g["name"].split("ins")[1]))
        banded, free = cases.yardstick(g)[0], cases.yardstick(g, band=600)[0]
        assert banded["d0"] == 0 and free["status"] & 2 == 0, g["name"]
        if gap == W + 1:
            assert banded["score"] < free["score"] and banded["status"] & 2, g["name"]
        elif gap < W:
            assert banded["score"] == free["score"] and banded["status"] & 2 == 0 and banded["ops"] == free["ops"], g["name"]
        if gap > 2 and gap <= W:
            assert (banded["n_del"], banded["n_ins"]) == ((gap, 0) if kind == "del" else (0, gap)), g["name"]
    groups = {g["name"]: g for g in cases.all_groups()}
    rnd = cases.yardstick(groups["random200"])
    assert len(rnd) == 200 and sum(1 for r in rnd if r["status"] & 2) < 20 and all(r["status"] & 1 == 0 for r in rnd)
    assert sum(1 for r in rnd if r["n_ins"] or r["n_del"]) > 50
    assert all(r["status"] & 1 for r in cases.yardstick(groups["rejected"]))
    (lo,), (hi,) = cases.yardstick(groups["identity900"]), cases.yardstick(groups["identity901"])
    assert lo["n_match"] == 90 == hi["n_match"] and lo["status"] & 1 == 0 and hi["status"] & 1 == 1
    assert cases.yardstick(groups["no-path"])[0]["score"] == ref.NO_SCORE
    ends = cases.yardstick(groups["ends"])
    assert ends[0]["ops"].startswith("IM") and ends[1]["ops"].endswith("MI") and ends[2]["ops"][:2] == "IM"
    assert ends[4]["ops"] == "I" * 7 + "M" * 257 + "I" * 9 and ends[4]["d0"] == -7
    # the tie cases have several optimal paths: flipping the H preference changes the ops of at least one of them
    assert any(r["n_ins"] or r["n_del"] for r in cases.yardstick(groups["ties"]))


def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(REPO, "scripts", "anchor_msa.py"), *args], capture_output=True, text=True)


def test_command_line_errors(tmp_path):
    seed, empty = tmp_path / "seed.fa", tmp_path / "empty.fa"
    seed.write_text(">a\nACGTACGTACGTACGT\n>b\nACGTACGTACGTACGA\n")
    empty.write_text("")
    out = str(tmp_path / "out.fa")
    assert _cli().returncode == 2                                                        # required flags missing
    assert _cli("-s", str(seed), "-i", str(seed), "-o", out, "--band", "256").returncode == 2
    assert _cli("-s", str(seed), "-i", str(seed), "-o", out, "--bogus").returncode == 2
    assert _cli("-s", str(seed), "-i", str(seed), "-o", out, "--min-identity", "1.5").returncode == 2
    assert _cli("-s", str(seed), "-i", str(tmp_path / "missing.fa"), "-o", out).returncode == 1
    assert _cli("-s", str(tmp_path / "missing.fa"), "-i", str(seed), "-o", out).returncode == 1
    r = _cli("-s", str(seed), "-i", str(empty), "-o", out)
    assert r.returncode == 1 and "empty.fa" in r.stderr
    ragged = tmp_path / "ragged.fa"
    ragged.write_text(">a\nACGT\n>b\nACG\n")
    assert _cli("-s", str(ragged), "-i", str(seed), "-o", out).returncode == 1
    assert not os.path.exists(out)


def test_api_refuses_bad_queries_before_any_launch(tmp_path):
    from multiprime_amd.anchor import AnchoredAlignment
    seed, long_q, empty_q = tmp_path / "seed.fa", tmp_path / "long.fa", tmp_path / "emptyq.fa"
    seed.write_text(">a\nACGTACGTACGTACGT\n")
    long_q.write_text(">ok\nACGT\n>toolong\n" + "A" * 32768 + "\n")
    empty_q.write_text(">ok\nACGT\n>nothing\n\n>last\nAC\n")
    with pytest.raises(ValueError, match="toolong"):
        AnchoredAlignment(str(seed), str(long_q), str(tmp_path / "o.fa")).load()
    with pytest.raises(ValueError, match="nothing"):
        AnchoredAlignment(str(seed), str(empty_q), str(tmp_path / "o.fa")).load()
    with pytest.raises(ValueError):
        AnchoredAlignment(str(seed), str(seed), str(tmp_path / "o.fa"), band=256)
    with pytest.raises(RuntimeError):
        AnchoredAlignment(str(seed), str(seed), str(tmp_path / "o.fa")).rows()
