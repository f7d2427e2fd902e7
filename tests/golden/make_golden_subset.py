#!/usr/bin/env python3
"""Golden recordings of the reference's global-optimum selection (`-m multiPrime2` of test_data/global_optimum/multiPrime2-core_V2.py,
"V2"): calls of its get_Y_position with their inputs and results, produced by RUNNING the unmodified script's class (imported by path; no
reference source is copied).

V2 hands a Python `set` of strings to itertools.combinations, so the winner among equal totals depends on PYTHONHASHSEED.  The one thing
this generator changes is the ORDER of that set: the module's `itertools` name is replaced by a stand-in whose combinations() sorts its
input by (position, A<C<G<T) first.  That order is the rule the project adopts.

Recorded, into tests/golden/subset_msa1000.json.gz:
  windows   on test_data/1000_fasta.msa at `-n 4 -v 1` and `-n 3 -v 2` (every other flag at V2's default): every window whose NM and MM
            seeds differ, every window that hit the |T| < dn rule, and every eighth of the rest.  Per call: seed, the items of `cover` in
            dictionary order, cover_number, N, v -> primer, count.
  direct    a handful of direct calls of get_Y_position on constructed covers (all counts 1, no IUPAC code: a total cannot exceed
            cover_number) that make its early exit fire.

Usage: python tests/golden/make_golden_subset.py
"""
import gzip
import importlib.util
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
V2 = os.path.join(REF, "test_data", "global_optimum", "multiPrime2-core_V2.py")
MSA = os.path.join(REF, "test_data", "1000_fasta.msa")
SETTINGS = [dict(n=4, v=1), dict(n=3, v=2)]


class SortedItertools:
    """`itertools` as V2 sees it: combinations() of the element strings "position|base" in the adopted order."""

    @staticmethod
    def combinations(iterable, r):
        return itertools.combinations(sorted(iterable, key=lambda e: (int(e.split("|")[0]), "ACGT".index(e.split("|")[1]))), r)

    def __getattr__(self, name):
        return getattr(itertools, name)


def load_v2():
    spec = importlib.util.spec_from_file_location("mpcore2_v2", V2)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.itertools = SortedItertools()
    return mod


class Sink:
    def put(self, item):
        pass


def record_windows(mod, seq_dict, total, n, v):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import subset_ref                                       # only to find the windows that hit the |T| < dn rule
    app = mod.NN_degenerate(Seq_dict=seq_dict, Total_sequence_number=total, number_of_dege_bases=n, variation=v, method="multiPrime2",
                            nproc=1, outfile=os.devnull)
    app.resQ = Sink()
    calls = []
    inner = app.get_Y_position

    def spy(optimal_primer, all_primers, cover_number, cover):
        items = [[key, int(val)] for key, val in cover.items()]
        primer, count = inner(optimal_primer, all_primers, cover_number, cover)
        calls.append({"seed": optimal_primer, "cover": items, "cover_number": int(cover_number), "N": n, "v": v, "primer": primer,
                      "count": int(count)})
        return primer, count

    app.get_Y_position = spy
    windows = []
    for pos in range(app.start_position, app.stop_position - app.primer_length):
        first = len(calls)
        app.get_primers(seq_dict, pos)
        if len(calls) > first:
            windows.append((pos, calls[first:]))
    kept, plain, n_calls = [], 0, 0
    for pos, cs in windows:
        n_calls += len(cs)
        two = len(cs) == 2
        short = False
        for c in cs:
            recs = subset_ref.records(c["seed"], c["cover"])
            short |= any(len(subset_ref.step(recs, dn, v, c["cover_number"])[0]) < dn for dn in range(2, n + 1))
        if not two and not short:
            plain += 1
            if plain % 8:
                continue
        for i, c in enumerate(cs):
            kept.append(dict(c, position=pos, role=("NM", "MM")[i] if two else "one"))
    print(f"-n {n} -v {v}: {len(windows)} windows, {n_calls} calls, {len(kept)} kept", flush=True)
    return kept


def direct_calls(mod):
    """Constructed covers that make V2's early exit fire; the seed is never a key, every count is 1."""
    cases = [
        # one substitution covers both records at the first rank of the first step
        dict(seed="AAAAAAAA", keys=["CCAAAAAA", "CACAAAAA"], N=3, v=1),
        # the covering substitution is not the first element: ranks before it set max_count first
        dict(seed="AAAAAAAA", keys=["ACCAAAAA", "AACCAAAA", "CACAAAAA"], N=3, v=1),
        # an earlier step sets a subset (one substitution covers one record), a later step (two substitutions) ends the search
        dict(seed="AAAAAAAA", keys=["CCAAAAAA", "AACCAAAA", "CACACAAA"], N=4, v=1),
        # the same with v = 2 and a longer seed
        dict(seed="AAAAAAAAAAAA", keys=["CCCAAAAAAAAA", "AAACCCAAAAAA", "CAACAACCAAAA"], N=4, v=2),
        # a gap element: it counts as a mismatch and merging it changes nothing
        dict(seed="ACGTACGT", keys=["-CGTACGA", "CCGTACGA"], N=3, v=1),
    ]
    out = []
    for case in cases:
        app = object.__new__(mod.NN_degenerate)
        app.number_of_dege_bases, app.variation = case["N"], case["v"]
        cover = {key: 1 for key in case["keys"]}
        primer, count = app.get_Y_position(case["seed"], set(cover), len(cover), cover)
        out.append({"seed": case["seed"], "cover": [[key, 1] for key in case["keys"]], "cover_number": len(cover), "N": case["N"], "v": case["v"],
                    "primer": primer, "count": int(count), "role": "direct"})
        print("direct:", case["seed"], case["keys"], "->", primer, count, flush=True)
    return out


def main():
    mod = load_v2()
    seq_dict, total = mod.parse_seq(MSA)
    out = {"source": "multiPrime2-core_V2.py get_Y_position, combinations in (position, A<C<G<T) order", "input": "test_data/1000_fasta.msa",
           "windows": [], "direct": direct_calls(mod)}
    for s in SETTINGS:
        out["windows"] += record_windows(mod, seq_dict, total, s["n"], s["v"])
    path = os.path.join(HERE, "subset_msa1000.json.gz")
    with open(path, "wb") as f:
        f.write(gzip.compress(json.dumps(out, sort_keys=True, separators=(",", ":")).encode(), 9, mtime=0))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
