"""Off-target-aware set selection (scripts/get_Maxprimerset.py -r): how many products every ordered pair of candidate
primers gives on a background, looked up by the greedy set cover of maxset.py.

The rule is the one at the head of include/mprime_setscreen.h — what get_Maxprimerset_V3.py spells out (V3:535-548: all
combinations of a forward and a reverse site on one background sequence, lo < stop - start + 1 < hi, counted over the growing
set); V3 itself cannot run.  The mapper is this build's k-mismatch scan (mp_kmm_scan's rule), not bowtie2.  The device keeps the
primers' sites and joins only what an `ensure` adds (csrc/setscreen.hip); `counts` is a dict lookup.
"""
from __future__ import annotations

import os

import numpy as np

from . import iupac
from .panel import TERM_MATCH

PATTERN_MIN_LEN, PATTERN_MAX_LEN = 4, 64           # mprime.h: MP_PATTERN_MAX_LEN
_IUPAC = set("ACGTRYMKSWHBVDN")


class RefusedPrimer(ValueError):
    """A primer the screen cannot take; the message names it."""


def term_of(primer: str, dist: int) -> str:
    return primer if dist == 0 or len(primer) <= dist else primer[-dist:]


def reads_of(primer: str, dist: int) -> list[str]:
    """The reads of a primer: the expansions of its last `dist` letters (all of it when dist == 0), in expansion order."""
    if not primer or not set(primer) <= _IUPAC:
        raise RefusedPrimer(f"primer {primer!r} holds letters outside the upper-case IUPAC nucleotide codes")
    term = term_of(primer, dist)
    if not PATTERN_MIN_LEN <= len(term) <= PATTERN_MAX_LEN:
        raise RefusedPrimer(f"primer {primer!r}: its term of {len(term)} bases is outside {PATTERN_MIN_LEN}..{PATTERN_MAX_LEN} "
                            "(limit of this build's scan, see INTEGRATION.md)")
    return iupac.expand(term)


def load_background(path):
    """(data, row_off) of a background FASTA; ValueError with the file's name when it is missing or holds no base."""
    if not path or not os.path.isfile(path):
        raise ValueError(f"background {path!r} does not exist")
    if os.path.getsize(path) == 0:
        raise ValueError(f"background {path!r} is empty")
    from .host import Fasta
    data, row_off = Fasta(str(path)).rows()
    if len(row_off) < 2 or row_off[-1] == row_off[0]:
        raise ValueError(f"background {path!r} is empty")
    return data, row_off


class OffTargetExaminer:
    """Pair counts of the primers seen so far.  With `table` ({(A, B): products(A -> B)} over primer strings, missing = 0) nothing
    touches a device: the greedy logic can run on precomputed counts."""

    def __init__(self, ctx=None, background=None, lo: int = 150, hi: int = 2000, dist: int = 12, mismatches: int = 1, *, table=None):
        self.lo, self.hi, self.dist, self.mismatches = lo, hi, dist, mismatches
        self.ids = {}                     # primer string -> global id
        self.names = []
        self.pairs = {}                   # (A, B) -> products(A -> B), non-zero only
        self.stats = {"adds": 0, "scan_ms": 0.0, "bin_ms": 0.0, "join_ms": 0.0, "per_add": []}
        self.injected = table is not None
        self.ctx = None
        if self.injected:
            self.pairs = {k: int(v) for k, v in table.items() if v}
            return
        data, row_off = load_background(background) if isinstance(background, (str, os.PathLike)) else background
        ctx.seq_load(data, row_off)
        ctx.setscreen_begin(lo, hi, mismatches, TERM_MATCH)
        self.ctx = ctx

    def ensure(self, primers):
        """Screen the primers not seen yet, in one add."""
        new = [p for p in dict.fromkeys(primers) if p not in self.ids]
        if not new:
            return
        reads = [reads_of(p, self.dist) for p in new]             # (refuses before anything is launched)
        first = len(self.names)
        for p in new:
            self.ids[p] = len(self.names)
            self.names.append(p)
        if self.injected:
            return
        flat = [r for rs in reads for r in rs]
        codes = iupac.MASK_LUT[np.frombuffer("".join(flat).encode(), np.uint8)]
        off = np.zeros(len(flat) + 1, np.int32)
        np.cumsum([len(r) for r in flat], out=off[1:])
        read_primer = np.repeat(np.arange(first, first + len(new), dtype=np.int32), [len(rs) for rs in reads])
        triples, (ms, _) = self.ctx.setscreen_add(codes, off, read_primer, with_stats=True)
        for a, b, n in triples.tolist():
            self.pairs[(self.names[a], self.names[b])] = n
        self.stats["adds"] += 1
        self.stats["per_add"].append((len(new), len(flat), ms["scan_ms"], ms["bin_ms"], ms["join_ms"]))
        for k in ("scan_ms", "bin_ms", "join_ms"):
            self.stats[k] += ms[k]

    def products(self, a: str, b: str) -> int:
        return self.pairs.get((a, b), 0)

    def counts(self, f: str, r: str, selected) -> tuple[int, int]:
        """(own, cross) of the candidate pair against the selected primer strings; O(|selected|)."""
        if f not in self.ids or r not in self.ids:
            raise KeyError("counts() of a primer that was never ensured")
        new = [f] if f == r else [f, r]
        own = sum(self.products(a, b) for a in new for b in new)
        cross = sum(self.products(a, b) + self.products(b, a) for a in new for b in selected if b not in new)
        return own, cross

    def close(self):
        if self.ctx is not None:
            self.ctx.setscreen_end()
            self.ctx = None
