"""The subset search of `-m multiPrime2` on the device (csrc/subset.hip behind include/mprime_subset.h) against the plain-Python model of
tests/subset_ref.py: the recorded windows of the reference, the constructed edge cases of tests/subset_cases.py, and the whole core step
with method="multiPrime2" against the same run with the selection taken from the model."""
import os

import numpy as np
import pytest

import subset_cases as cases
import subset_ref as ref
from conftest import golden_input, load_gz_json
from test_subset import model_steps, seeds_of

pytestmark = pytest.mark.gpu

STEP_KEYS = ("t_mask", "n_admitted", "best_total", "best_rank", "exit_rank", "pre_total")


@pytest.fixture(scope="module")
def ctx(hip_lib):
    assert hip_lib.backend == "hip"
    c = hip_lib.context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return load_gz_json("subset_msa1000.json.gz")


def words_of(kmers, k):
    """Window words (b0, b1, g planes) of k-mer strings: [3][n], uint32 up to k = 31, uint64 above."""
    out = np.zeros((3, len(kmers)), np.uint64)
    for i, u in enumerate(kmers):
        for j, ch in enumerate(u):
            if ch == "-":
                out[2, i] |= np.uint64(1 << j)
            else:
                b = "ACGT".index(ch)
                out[0, i] |= np.uint64((b & 1) << j)
                out[1, i] |= np.uint64((b >> 1) << j)
    return out.astype(np.uint32 if k <= 31 else np.uint64)


def arrays_of(case):
    off, kmers, counts = [0], [], []
    for w in case["windows"]:
        kmers += [u for u, _ in w]
        counts += [n for _, n in w]
        off.append(len(kmers))
    # a window's table holds every k-mer; `cover` is those with at most v gaps (the others are gap_sequence keys)
    covers = [[(u, n) for u, n in w if u.count("-") <= case["v"]] for w in case["windows"]]
    calls = [{"seed": seed, "cover": covers[w], "cover_number": cn, "N": case["N"], "v": case["v"]} for w, seed, cn in case["searches"]]
    return np.asarray(off, np.int64), words_of(kmers, case["k"]), np.asarray(counts, np.int64), calls


def run_explicit(ctx, case):
    from multiprime_amd import subset
    off, words, counts, calls = arrays_of(case)
    got = subset.search(ctx, case["k"], case["v"], case["N"], off, words, counts, [w for w, _, _ in case["searches"]], seeds_of(calls),
                        [c["cover_number"] for c in calls])
    return got, calls


def check_against_model(got, calls, k, N):
    """Every per-step result, then the replayed subset, count and merged primer."""
    from multiprime_amd import host, iupac, subset
    want = model_steps(calls) if N > 1 else None
    if want is not None:
        for key in STEP_KEYS:
            assert np.array_equal(got[key], want[key]), (key, got[key].tolist(), want[key].tolist())
    masks, counts, codes = subset.replay(host.dll(), k, N, seeds_of(calls), [c["cover_number"] for c in calls], got)
    primers = iupac.strings_of(iupac.SYMBOL_LUT[codes])
    picked = []
    for i, c in enumerate(calls):
        chosen, count, primer = ref.select(c["seed"], c["cover"], c["cover_number"], N, c["v"])
        assert tuple(int(x) for x in masks[i]) == ref.mask_of(chosen) and (primers[i], int(counts[i])) == (primer, count), (i, c["seed"], primer)
        picked.append((primers[i], int(counts[i])))
    return picked


def test_recorded_windows_explicit(ctx, golden):
    groups = {}
    for c in golden["windows"] + golden["direct"]:
        groups.setdefault((len(c["seed"]), c["N"], c["v"]), []).append(c)
    for (k, N, v), calls in groups.items():
        case = {"k": k, "v": v, "N": N, "windows": [c["cover"] for c in calls],
                "searches": [(i, c["seed"], c["cover_number"]) for i, c in enumerate(calls)]}
        got, mine = run_explicit(ctx, case)
        picked = check_against_model(got, mine, k, N)
        assert picked == [(c["primer"], c["count"]) for c in calls]              # ... which is what the reference returned


ALL = cases.all_cases()


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_constructed_case(ctx, case):
    got, calls = run_explicit(ctx, case)
    picked = check_against_model(got, calls, case["k"], case["N"])
    name = case["name"]
    if case["N"] == 1:
        assert picked == [(c["seed"], 0) for c in calls]                          # no step: the seed comes back
    if name.startswith("exit_at_1"):
        assert got["exit_rank"][0, 1] == int(name[8:]) and got["pre_total"][0, 1] == 2
    if name.startswith("equal_totals"):
        assert got["best_rank"][0, 1] == 10 and got["best_total"][0, 1] == 50    # rank 1500 has the same total in another workgroup
    if name == "optimum_at_last_rank":
        assert got["best_rank"][0, 1] == 2079
    if name == "optimum_at_rank_0":
        assert got["best_rank"][0, 1] == 0
    if name in ("T_64", "T_65"):
        assert bin(int(got["t_mask"][0, 1, 0])).count("1") + bin(int(got["t_mask"][0, 1, 1])).count("1") == int(name[2:])
    if name == "grid_k32_v1_N4":
        assert int(got["t_mask"][0, 2, 1]) >> 60                                   # element ids 124..127 in use
    if name == "nm_mm_tie":
        from multiprime_amd import host, subset
        assert picked[0][1] == picked[1][1] and picked[0][0] != picked[1][0]
        assert subset.choose(host.dll(), [0], [1], [picked[0][1], picked[1][1]]).tolist() == [0]
    if name == "counts_near_2_31":
        assert picked[0][1] == 2 ** 32 - 4


def test_entry_order_does_not_matter(ctx):
    case = next(c for c in ALL if c["name"] == "ragged_33_searches")
    got, _ = run_explicit(ctx, case)
    turned = dict(case, windows=[w[::-1] for w in case["windows"]])
    again, _ = run_explicit(ctx, turned)
    for key in STEP_KEYS:
        assert np.array_equal(got[key], again[key]), key


@pytest.mark.parametrize("case,message", cases.refusal_cases(), ids=[c["name"] for c, _ in cases.refusal_cases()])
def test_refusals(ctx, case, message):
    from multiprime_amd._abi import MprimeError
    with pytest.raises(MprimeError) as e:
        run_explicit(ctx, case)
    assert e.value.code == -1 and message in str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole step on a slice of the sample alignment
# ---------------------------------------------------------------------------------------------------------------------------------
COLUMNS = (300, 400)      # of tests/golden/inputs/1000_fasta.msa: the reference's first window with two different seeds starts at 328
FLAGS = dict(primer_length=18, coverage=0.6, number_of_dege_bases=3, score_of_dege_bases=10, product_len=30, position="1,2,-1", variation=1,
             raw_entropy_threshold=3.6, distance=4, GC="0.2,0.7", nproc=1)


@pytest.fixture(scope="module")
def slice_file(tmp_path_factory):
    records, name = [], None
    for line in golden_input("1000_fasta.msa").decode().splitlines():
        if line.startswith(">"):
            name = line
            records.append([name, ""])
        elif name is not None:
            records[-1][1] += line.strip()
    path = tmp_path_factory.mktemp("subset") / "slice.msa"
    path.write_text("".join(f"{n}\n{s[COLUMNS[0]:COLUMNS[1]]}\n" for n, s in records))
    return str(path)


def outputs(out):
    return [open(out + ext, "rb").read() for ext in ("", ".non_coverage_seq_id_json", ".gap_seq_id_json")]


def test_whole_step_equals_the_models_selection(hip_lib, slice_file, tmp_path):
    from multiprime_amd import host, iupac, subset
    from multiprime_amd.core import NN_degenerate

    N, v, k = FLAGS["number_of_dege_bases"], FLAGS["variation"], FLAGS["primer_length"]
    seen = {}

    class ModelSelection(NN_degenerate):
        """The same step with the final primers chosen by the model from the plan's ordered cover tables; the explicit form is run on the
        same tables beside it and must agree step by step."""

        def _select_by_subsets(self, plan):
            wins, s_window, s_seed, s_cover, nm, mm = subset.plan_searches(plan)
            tables = {}
            for w in wins.tolist():
                codes, counts, _ = plan.window_table(w, 0)
                tables[w] = list(zip(iupac.strings_of(iupac.SYMBOL_LUT[codes]), counts.tolist()))
            seeds = ["".join("ACGT"[b] for b in row) for row in s_seed.tolist()]
            results = [ref.select(seeds[i], tables[int(w)], int(s_cover[i]), N, v) for i, w in enumerate(s_window)]
            final = [ref.pick(results[a], results[b] if b >= 0 else None)[2] for a, b in zip(nm.tolist(), mm.tolist())]
            seen["two_seeds"] = int((mm >= 0).sum())
            seen["differ"] = sum(results[a][2] != results[b][2] for a, b in zip(nm.tolist(), mm.tolist()) if b >= 0)
            order = {w: i for i, w in enumerate(wins.tolist())}
            case = {"k": k, "v": v, "N": N, "windows": [tables[w] for w in wins.tolist()],
                    "searches": [(order[int(w)], seeds[i], int(s_cover[i])) for i, w in enumerate(s_window)]}
            got, calls = run_explicit(self.ctx, case)
            check_against_model(got, calls, k, N)
            codes = iupac.MASK_LUT[np.frombuffer("".join(final).encode(), np.uint8)].reshape(len(final), k)
            ev = self.ctx.eval_candidates(wins, codes, self._sF, self._sR)
            subset.finish_given(plan, codes, ev)
            return ev

    outs = {}
    for name, cls, kw in (("device", NN_degenerate, dict(method="multiPrime2")), ("model", ModelSelection, dict(method="multiPrime2")),
                          ("chain", NN_degenerate, dict(method="multiPrime1")), ("default", NN_degenerate, {})):
        out = str(tmp_path / (name + ".tsv"))
        app = cls(seq_file=slice_file, outfile=out, library=hip_lib, **FLAGS, **kw)
        try:
            app.run()
            if name == "device":
                stats = dict(app.stats)
                # the resident form against the explicit form on the same tables: the context still holds the histograms
                wins, s_window, s_seed, s_cover, _, _ = subset.plan_searches(app.plan)
                resident = subset.search_resident(app.ctx, N, s_window, s_seed, s_cover, extra=app._extra)
                off, words, count, _ = app.ctx.window_unique()
                off, words, count = with_extras(off, words, count, app._extra)
                explicit = subset.search(app.ctx, k, v, N, off, words, count, s_window, s_seed, s_cover)
                for key in STEP_KEYS:
                    assert np.array_equal(resident[key], explicit[key]), key
        finally:
            app.ctx.close()
        outs[name] = outputs(out)
    assert seen["two_seeds"] >= 1 and stats["subset_searches"] == stats["windows_planned"] + seen["two_seeds"]
    assert outs["device"] == outs["model"]
    assert outs["chain"] == outs["default"]
    assert len(outs["device"][0].splitlines()) > 1


def with_extras(off, words, count, extra):
    """The histogram entries with the extra entries (count 1 each) appended to their windows."""
    if extra is None:
        return off, words, count.astype(np.int64)
    x_win, x_words = extra
    W = len(off) - 1
    new_off, cols, cnts = [0], [], []
    for w in range(W):
        a, b = int(off[w]), int(off[w + 1])
        mine = np.nonzero(x_win == w)[0]
        cols.append(words[:, a:b])
        cols.append(x_words[mine].T.astype(words.dtype))
        cnts += count[a:b].tolist() + [1] * len(mine)
        new_off.append(len(cnts))
    return np.asarray(new_off, np.int64), np.ascontiguousarray(np.concatenate(cols, axis=1)), np.asarray(cnts, np.int64)


def test_batch_and_flags_run_method_2(hip_lib, slice_file, tmp_path):
    """--batch, --no-json and --bitsets with -m multiPrime2 through the command line's batch runner: same TSV as the class."""
    from multiprime_amd import cli
    from multiprime_amd.core import NN_degenerate
    out = str(tmp_path / "direct.tsv")
    app = NN_degenerate(seq_file=slice_file, outfile=out, library=hip_lib, method="multiPrime2", write_json=False, **FLAGS)
    try:
        app.run()
    finally:
        app.ctx.close()
    want = open(out, "rb").read()
    assert not os.path.exists(out + ".gap_seq_id_json")
    batch = tmp_path / "batch.txt"
    batch.write_text(f"{slice_file}\t{tmp_path / 'b1.tsv'}\n{slice_file}\t{tmp_path / 'b2.tsv'}\n")
    args = cli.parse_args(["--batch", str(batch), "--batch-workers", "1", "-m", "multiPrime2", "-l", "18", "-f", "0.6", "-n", "3", "-d", "10", "-s", "30",
                           "-c", "1,2,-1", "-v", "1", "-e", "3.6", "-a", "4", "-g", "0.2,0.7", "-p", "1", "--no-json", "--bitsets"])
    cli._run_batch(args, 0, 1, 0)
    for name in ("b1.tsv", "b2.tsv"):
        assert open(tmp_path / name, "rb").read() == want
        assert os.path.exists(str(tmp_path / name) + ".coverage_bitsets.npz") and not os.path.exists(str(tmp_path / name) + ".gap_seq_id_json")
