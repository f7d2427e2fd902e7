"""Pair coverage — popcount(set_a[i] | set_b[j]) — called directly, against a plain numpy model (unpack the words into bits, OR,
sum; bit assignments applied one at a time): the free form mp_pair_coverage (pair_coverage_kernel) and the resident coverage masks
(mp_eval_masks_resident, mp_masks_set_bits, mp_masks_fetch, mp_pair_coverage_resident: mask_set_kernel, mask_pair_kernel and the
three producers of the masks' tail word).  Inside Primers_filter the counts pass a coverage threshold before anything is compared;
here every count is compared as it is.

Shapes: 1 .. 129 words (the lane loop takes its second trip from 65 words on), pair counts off the four-pairs-per-workgroup grid,
row counts 5 .. 4097 (4097 rows = 65 words at a stride of 68), all rows of one word assigned in one launch, and the check that a
mask with every row set counts n_rows, not the padded row count.

CPU leg: the checker against the model.  GPU leg (`-m gpu`): the HIP library against the model and against the checker."""
import numpy as np
import pytest

from multiprime_amd import iupac
from multiprime_amd._abi import MprimeError
from test_hip_parity import chain_candidates, fuzz_msa


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def bits_of(words):
    """uint64 [..., n_words] -> uint8 [..., 64 n_words], bit j of word w at 64 w + j."""
    words = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")


def words_of(bits):
    return np.packbits(bits, axis=-1, bitorder="little").view("<u8").astype(np.uint64)


def model_coverage(a, b, pairs):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return (bits_of(a)[pairs[:, 0]] | bits_of(b)[pairs[:, 1]]).sum(axis=-1, dtype=np.int64).astype(np.int32)


def model_set_bits(not_f, not_r, cand, row, which, value):
    planes = [bits_of(not_f), bits_of(not_r)]
    for c, r, w, v in zip(cand, row, which, value):           # one at a time, in the order given
        planes[w][c, r] = v
    return words_of(planes[0]), words_of(planes[1])


# ---- the free form -----------------------------------------------------------------------------------------------------------------
N_WORDS = (1, 63, 64, 65, 128, 129)
N_SETS = (1, 7, 40)
N_PAIRS = (1, 3, 4, 5, 1001)


def mixed_pairs(rng, n_sets, n_pairs, falling):
    pairs = rng.integers(0, n_sets, size=(n_pairs, 2)).astype(np.int32)
    pairs[0] = int(rng.integers(0, n_sets))                    # a pair (i, i)
    if n_pairs >= 3:
        pairs[2] = pairs[1]                                    # a repeated pair
    if falling:
        pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))[::-1]]
    return np.ascontiguousarray(pairs)


def free_cases(n_words):
    """(label, sets_a, sets_b, pairs, the count known beforehand or None)"""
    rng = np.random.default_rng(1000 + n_words)
    top = np.uint64(1) << np.uint64(63)
    for n_sets in N_SETS:
        for n_pairs in N_PAIRS:
            a = rng.integers(0, 2 ** 64, size=(n_sets, n_words), dtype=np.uint64)
            b = rng.integers(0, 2 ** 64, size=(n_sets, n_words), dtype=np.uint64)
            zeros, ones = np.zeros_like(a), np.full_like(a, np.uint64(2 ** 64 - 1))
            pairs = mixed_pairs(rng, n_sets, n_pairs, falling=False)
            falling = mixed_pairs(rng, n_sets, n_pairs, falling=True)
            one = zeros.copy()
            one[n_sets // 2, n_words - 1] = top                # the bit 64 n_words - 1 of one set only
            yield f"random {n_sets} {n_pairs}", a, b, pairs, None
            yield f"random, falling order {n_sets} {n_pairs}", a, b, falling, None
            yield f"one array twice {n_sets} {n_pairs}", a, a, pairs, None
            yield f"zeros {n_sets} {n_pairs}", zeros, zeros, pairs, np.zeros(n_pairs, np.int32)
            yield f"ones {n_sets} {n_pairs}", ones, zeros, pairs, np.full(n_pairs, 64 * n_words, np.int32)
            yield f"ones in both {n_sets} {n_pairs}", ones, ones, falling, np.full(n_pairs, 64 * n_words, np.int32)
            yield f"top bit in a {n_sets} {n_pairs}", one, zeros, pairs, (pairs[:, 0] == n_sets // 2).astype(np.int32)
            yield f"top bit in b {n_sets} {n_pairs}", zeros, one, falling, (falling[:, 1] == n_sets // 2).astype(np.int32)


def check_free_form(libs, n_words):
    ctxs = [lib.context(0) for lib in libs]
    try:
        for label, a, b, pairs, known in free_cases(n_words):
            want = model_coverage(a, b, pairs)
            if known is not None:
                assert np.array_equal(want, known), label
            for ctx in ctxs:
                got = ctx.pair_coverage(a, b, pairs)
                assert got.dtype == np.int32 and np.array_equal(got, want), (label, ctx.lib.backend)
    finally:
        for ctx in ctxs:
            ctx.close()


def check_free_form_refusals(lib):
    ctx = lib.context(0)
    try:
        a = np.arange(14, dtype=np.uint64).reshape(7, 2)
        assert ctx.pair_coverage(a, a, np.zeros((0, 2), np.int32)).shape == (0,)
        for bad in ([[0, -1]], [[-1, 0]], [[7, 0]], [[0, 7]], [[0, 0], [1, 1], [6, 7]]):
            with pytest.raises(MprimeError, match="out of range"):
                ctx.pair_coverage(a, a, np.asarray(bad, np.int32))
        assert ctx.pair_coverage(a, a, np.asarray([[6, 6]], np.int32)).tolist() == [5]      # the words 12 and 13: 2 + 3 bits
    finally:
        ctx.close()


@pytest.mark.parametrize("n_words", N_WORDS)
def test_checker_free_form_equals_the_model(oracle_lib, n_words):
    check_free_form([oracle_lib], n_words)


def test_checker_free_form_refusals(oracle_lib):
    check_free_form_refusals(oracle_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("n_words", N_WORDS)
def test_hip_free_form_equals_the_model_and_the_checker(hip_lib, oracle_lib, n_words):
    check_free_form([hip_lib, oracle_lib], n_words)


@pytest.mark.gpu
def test_hip_free_form_refusals(hip_lib):
    check_free_form_refusals(hip_lib)


# ---- the resident form -------------------------------------------------------------------------------------------------------------
ROWS = (5, 64, 65, 257, 4097)
# k, v, environment: the bit-sliced producer, the row kernel by request, the row kernel because v > 3, the 64-bit word kernels
PRODUCERS = {"bits": (18, 1, {}), "rows": (18, 1, {"MP_MASK_MODE": "rows"}), "v4": (18, 4, {}), "wide": (40, 2, {})}
L, P0 = 110, 3


def resident_case(n, producer):
    k, v, env = PRODUCERS[producer]
    data, off, _ = fuzz_msa(500 + n + k + v, n, L, ragged=False, p_gap=0.05, p_iupac=0.004)
    W = L - P0 - k - 2
    rng = np.random.default_rng(n * 5 + k + v)
    root = iupac.MASK_LUT[data[P0:L]]                          # the first row from the first window on: candidates that reach some rows
    root = np.where(np.isin(root, [1, 2, 4, 8]), root, 1).astype(np.uint8)
    cw, codes = chain_candidates(rng, root, W, k, "mixed")
    keep = np.sort(rng.permutation(len(cw))[:40])
    return dict(n=n, k=k, v=v, env=env, data=data, off=off, W=W, cw=cw[keep], codes=codes[keep], sF=0b1100,
                sR=sum(1 << y for y in (2, k - 3, k - 2)), rng=rng)


def assignments(rng, n, n_masks):
    """(cand, row, which, value): a few thousand, no bit with two values; exact duplicates; one whole word of one mask set and one
    cleared; rows 0, 63, 64 and n - 1 of both kinds of mask, set and cleared."""
    chosen, order = {}, []

    def add(c, r, w, v):
        if 0 <= r < n:
            v = chosen.setdefault((c, r, w), v)
            order.append((c, r, w, v))
    word = 1 if n > 128 else 0
    for r in range(64 * word, 64 * word + 64):
        add(1, r, 0, 1)                                        # every row of one word of one mask, set
        add(2, r, 1, 0)                                        # and of another, cleared
    for r in (0, 63, 64, n - 1):
        for w in (0, 1):
            add(3, r, w, 1)
            add(4, r, w, 0)
            add(n_masks - 1, r, w, (r + w) & 1)
    for _ in range(3000):
        c, r, w = int(rng.integers(0, n_masks)), int(rng.integers(0, n)), int(rng.integers(0, 2))
        add(c, r, w, (c + r + w) & 1)
    dup = [order[i] for i in rng.integers(0, len(order), size=200)]
    order = order + dup                                        # exact duplicates, apart from their first copies
    cand, row, which, value = (np.asarray(x) for x in zip(*order))
    return cand.astype(np.int32), row.astype(np.int32), which.astype(np.uint8), value.astype(np.uint8)


def run_resident(lib, case, monkeypatch):
    """The five steps on one library, each checked against the model; returns what two libraries must agree on."""
    n, rng = case["n"], np.random.default_rng(case["n"] + case["k"])
    nw = (n + 63) // 64
    ctx = lib.context(0)
    try:
        ctx.load_msa(case["data"], case["off"])
        ctx.build_windows(P0, case["W"], case["k"], case["v"])
        with monkeypatch.context() as m:
            for key, val in case["env"].items():
                m.setenv(key, val)
            ctx.eval_masks_resident(case["cw"], case["codes"], case["sF"], case["sR"])
        n_masks = len(case["cw"])
        # 1. the masks as computed
        nf, nr = ctx.masks_fetch()
        assert nf.shape == nr.shape == (n_masks, nw)
        out = [nf.copy(), nr.copy()]
        # 2. coverage of pairs: random, (i, i), repeats, a count off the multiple of four
        pairs = mixed_pairs(rng, n_masks, 37, falling=False)
        cov = ctx.pair_coverage_resident(pairs)
        assert np.array_equal(cov, model_coverage(nf, nr, pairs))
        assert np.array_equal(cov, ctx.pair_coverage(nf, nr, pairs))
        assert ctx.pair_coverage_resident(np.zeros((0, 2), np.int32)).shape == (0,)
        out.append(cov)
        # 3. single bits
        cand, row, which, value = assignments(rng, n, n_masks)
        assert len(cand) > 3000 and set(which.tolist()) == {0, 1} and set(value.tolist()) == {0, 1}
        ctx.masks_set_bits(cand, row, which, value)
        mf, mr = model_set_bits(nf, nr, cand, row, which, value)
        gf, gr = ctx.masks_fetch()
        assert np.array_equal(gf, mf) and np.array_equal(gr, mr)
        every = np.stack(np.meshgrid(np.arange(n_masks), np.arange(n_masks), indexing="ij"), -1).reshape(-1, 2)[::-1]      # 1600 pairs, falling
        assert np.array_equal(ctx.pair_coverage_resident(every), model_coverage(mf, mr, every))
        # 4. every row of one forward and one reverse mask: the count is n, whatever lies beyond row n - 1 of the padded masks
        rows = np.arange(n, dtype=np.int32)
        ctx.masks_set_bits(np.concatenate([np.zeros(n, np.int32), np.ones(n, np.int32)]), np.concatenate([rows, rows]),
                           np.concatenate([np.zeros(n, np.uint8), np.ones(n, np.uint8)]), np.ones(2 * n, np.uint8))
        tail = np.asarray([[0, 1], [0, 0], [1, 1], [0, n_masks - 1], [n_masks - 1, 1]], np.int32)
        cov = ctx.pair_coverage_resident(tail)
        assert cov[[0, 1, 2, 3]].tolist() == [n, n, n, n] and cov[4] == n, cov
        gf, gr = ctx.masks_fetch()
        assert bits_of(gf[0]).sum() == n and bits_of(gr[1]).sum() == n
        assert np.array_equal(cov, model_coverage(gf, gr, tail))
        out.append(cov)
        # refusals of the assignments
        one = (np.zeros(1, np.uint8), np.ones(1, np.uint8))
        for c, r in ((0, n), (n_masks, 0), (0, -1), (-1, 0)):
            with pytest.raises(MprimeError, match="out of range"):
                ctx.masks_set_bits(np.asarray([c], np.int32), np.asarray([r], np.int32), *one)
        # 5. a second evaluation with fewer candidates replaces the masks
        last = np.asarray([[n_masks - 1, 0]], np.int32)
        assert ctx.pair_coverage_resident(last).shape == (1,)
        ctx.eval_masks_resident(case["cw"][:10], case["codes"][:10], case["sF"], case["sR"])
        with pytest.raises(MprimeError, match="out of range"):
            ctx.pair_coverage_resident(last)
        sf, sr = ctx.masks_fetch()
        assert sf.shape == (10, nw)
        few = mixed_pairs(rng, 10, 9, falling=True)
        cov = ctx.pair_coverage_resident(few)
        assert np.array_equal(cov, model_coverage(sf, sr, few))
        return out + [sf.copy(), sr.copy(), cov]
    finally:
        ctx.close()


def check_no_resident_masks(lib):
    ctx = lib.context(0)
    try:
        with pytest.raises(MprimeError, match="no resident masks"):
            ctx.pair_coverage_resident(np.asarray([[0, 0]], np.int32))
        with pytest.raises(MprimeError, match="no resident masks"):
            ctx.masks_set_bits(np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.uint8), np.ones(1, np.uint8))
        ctx.masks_set_bits(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint8))      # n == 0: nothing to do
    finally:
        ctx.close()


_CHECKER = {}


def checker_resident(oracle_lib, n, producer, monkeypatch):
    if (n, producer) not in _CHECKER:
        _CHECKER[n, producer] = run_resident(oracle_lib, resident_case(n, producer), monkeypatch)
    return _CHECKER[n, producer]


@pytest.mark.parametrize("producer", list(PRODUCERS))
@pytest.mark.parametrize("n", ROWS)
def test_checker_resident_masks_equal_the_model(oracle_lib, monkeypatch, n, producer):
    out = checker_resident(oracle_lib, n, producer, monkeypatch)
    for masks in out[:2]:                                               # rows a primer reaches and rows it does not
        assert bits_of(masks)[:, :n].any() and not bits_of(masks)[:, :n].all()


def test_checker_refuses_without_resident_masks(oracle_lib):
    check_no_resident_masks(oracle_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("producer", list(PRODUCERS))
@pytest.mark.parametrize("n", ROWS)
def test_hip_resident_masks_equal_the_model_and_the_checker(hip_lib, oracle_lib, monkeypatch, n, producer):
    want = checker_resident(oracle_lib, n, producer, monkeypatch)
    got = run_resident(hip_lib, resident_case(n, producer), monkeypatch)
    for step, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(x, y), f"result {step} differs from the checker's"


@pytest.mark.gpu
def test_hip_refuses_without_resident_masks(hip_lib):
    check_no_resident_masks(hip_lib)
