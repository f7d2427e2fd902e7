"""ctypes binding of include/mprime_subset.h — the global-optimum degenerate positions of the core step (`-m multiPrime2` of the
reference's test_data/global_optimum/multiPrime2-core_V2.py, get_Y_position / remove_elements): per window seed, all subsets of
(position, base) substitutions of a given size are searched on the device (csrc/subset.hip), the step rules are replayed on the host.
Served by libmprime_hip.so only; there is no fall-back.  The checker is the plain-Python model tests/subset_ref.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import MprimeError, _ptr

_p = C.c_void_p
MAX_K = 32

SUBSET_SYMBOLS = [
    ("mp_subset_search", C.c_int, [_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _p, _p, _p, C.c_int32, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    ("mp_subset_search_resident", C.c_int, [_p, C.c_int32, C.c_int64, _p, _p, C.c_int32, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    ("mp_subset_timing", C.c_int, [_p, _p]),
    ("mp_subset_replay", C.c_int, [C.c_int32, C.c_int32, C.c_int32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    ("mp_subset_choose", C.c_int, [C.c_int32, _p, _p, _p, _p]),
]

STEP_KEYS = ("t_mask", "n_admitted", "best_total", "best_rank", "exit_rank", "pre_total")


def bind(dll):
    """Declares the entry points on a loaded libmprime_hip.so; a library without them is an error, never a fall-back."""
    if getattr(dll, "_mp_subset_bound", False):
        return dll
    for name, res, args in SUBSET_SYMBOLS:
        if not hasattr(dll, name):
            raise MprimeError(-2, f"the library lacks {name} (include/mprime_subset.h): rebuild it")
        fn = getattr(dll, name)
        fn.restype = res
        fn.argtypes = args
    dll._mp_subset_bound = True
    return dll


def _steps(n_search, N):
    n = max(n_search * max(N - 1, 0), 1)
    return {"t_mask": np.zeros((n, 2), np.uint64), "n_admitted": np.zeros(n, np.int32), "best_total": np.zeros(n, np.int64),
            "best_rank": np.full(n, -1, np.int64), "exit_rank": np.full(n, -1, np.int64), "pre_total": np.zeros(n, np.int64)}


def _shape(out, n_search, N):
    st = max(N - 1, 0)
    return {key: val[: n_search * st].reshape((n_search, st) + val.shape[1:]) for key, val in out.items()}


def _searches(k, s_window, s_seed, s_cover):
    s_window = np.ascontiguousarray(s_window, dtype=np.int32)
    s_seed = np.ascontiguousarray(s_seed, dtype=np.uint8).reshape(len(s_window), k)
    s_cover = np.ascontiguousarray(s_cover, dtype=np.int64)
    if len(s_cover) != len(s_window):
        raise ValueError("one cover_number per search expected")
    return s_window, s_seed, s_cover


def search(ctx, k: int, v: int, N: int, win_off, words, counts, s_window, s_seed, s_cover):
    """Explicit form (mp_subset_search): per-step results as a dict of arrays [n_search][N - 1](...), keys STEP_KEYS."""
    d = bind(ctx.d)
    win_off = np.ascontiguousarray(win_off, dtype=np.int64)
    n = int(win_off[-1])
    words = np.ascontiguousarray(words, dtype=np.uint32 if k <= 31 else np.uint64).reshape(3, n)
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    if len(counts) != n:
        raise ValueError("one count per entry expected")
    s_window, s_seed, s_cover = _searches(k, s_window, s_seed, s_cover)
    out = _steps(len(s_window), N)
    ctx._ck(d.mp_subset_search(ctx.h, int(k), int(v), int(N), len(win_off) - 1, _ptr(win_off), _ptr(words), _ptr(counts), len(s_window),
                               _ptr(s_window), _ptr(s_seed), _ptr(s_cover), *[_ptr(out[key]) for key in STEP_KEYS]))
    return _shape(out, len(s_window), N)


def search_resident(ctx, N: int, s_window, s_seed, s_cover, extra=None):
    """Resident form (mp_subset_search_resident) over the histogram tables of ctx; extra = (windows, words [m][3]) of the IUPAC rows'
    expansions (host.expand_exception_words) or None."""
    d = bind(ctx.d)
    k = ctx.k
    s_window, s_seed, s_cover = _searches(k, s_window, s_seed, s_cover)
    x_win = x_words = None
    if extra is not None and len(extra[0]):
        x_win = np.ascontiguousarray(extra[0], dtype=np.int32)
        x_words = np.ascontiguousarray(extra[1], dtype=np.uint32 if k <= 31 else np.uint64).reshape(len(x_win), 3)
    out = _steps(len(s_window), N)
    ctx._ck(d.mp_subset_search_resident(ctx.h, int(N), 0 if x_win is None else len(x_win), _ptr(x_win), _ptr(x_words), len(s_window),
                                        _ptr(s_window), _ptr(s_seed), _ptr(s_cover), *[_ptr(out[key]) for key in STEP_KEYS]))
    return _shape(out, len(s_window), N)


def timing(ctx):
    """Device milliseconds (records, step sets, search) of the context's last search."""
    ms = np.zeros(3, np.float64)
    ctx._ck(bind(ctx.d).mp_subset_timing(ctx.h, _ptr(ms)))
    return ms


def replay(dll, k: int, N: int, s_seed, s_cover, steps):
    """Host replay (mp_subset_replay): (subset masks [n][2] uint64, max_count [n], merged primer codes [n][k])."""
    d = bind(dll)
    s_cover = np.ascontiguousarray(s_cover, dtype=np.int64)
    n = len(s_cover)
    s_seed = np.ascontiguousarray(s_seed, dtype=np.uint8).reshape(n, k)
    arr = {key: np.ascontiguousarray(steps[key]) for key in STEP_KEYS}
    if N > 1 and arr["best_total"].size != n * (N - 1):
        raise ValueError("per-step results of %d searches x %d steps expected" % (n, N - 1))
    subset = np.zeros((max(n, 1), 2), np.uint64)
    max_count = np.zeros(max(n, 1), np.int64)
    codes = np.zeros((max(n, 1), k), np.uint8)
    rc = d.mp_subset_replay(int(k), int(N), n, _ptr(s_seed), _ptr(s_cover), _ptr(arr["t_mask"]), _ptr(arr["best_total"]), _ptr(arr["best_rank"]),
                            _ptr(arr["exit_rank"]), _ptr(arr["pre_total"]), _ptr(subset), _ptr(max_count), _ptr(codes))
    if rc != 0:
        raise MprimeError(rc, "mp_subset_replay: bad arguments (k > 32, a base index above 3, or a rank outside its step)")
    return subset[:n], max_count[:n], codes[:n]


def choose(dll, nm, mm, max_count):
    """NM or MM per window (mp_subset_choose): the search index taken; mm[p] = -1 where the window has one seed."""
    d = bind(dll)
    nm = np.ascontiguousarray(nm, dtype=np.int32)
    mm = np.ascontiguousarray(mm, dtype=np.int32)
    max_count = np.ascontiguousarray(max_count, dtype=np.int64)
    chosen = np.zeros(max(len(nm), 1), np.int32)
    rc = d.mp_subset_choose(len(nm), _ptr(nm), _ptr(mm), _ptr(max_count), _ptr(chosen))
    if rc != 0:
        raise MprimeError(rc, "mp_subset_choose: bad arguments")
    return chosen[: len(nm)]


def plan_searches(plan):
    """The searches of a host.Plan: (windows of the planned windows, s_window, s_seed, s_cover, nm index, mm index per planned window)."""
    status, cover_number = plan.windows()[:2]
    wins = np.nonzero(status == 0)[0].astype(np.int32)
    s_window, s_seed, s_cover, nm, mm = [], [], [], [], []
    for w in wins.tolist():
        a, b, _, _ = plan.seeds(w)
        nm.append(len(s_window))
        s_window.append(w)
        s_seed.append(a)
        s_cover.append(int(cover_number[w]))
        if b is not None:
            mm.append(len(s_window))
            s_window.append(w)
            s_seed.append(b)
            s_cover.append(int(cover_number[w]))
        else:
            mm.append(-1)
    seeds = np.asarray(s_seed, np.uint8).reshape(len(s_window), plan.k)
    return wins, np.asarray(s_window, np.int32), seeds, np.asarray(s_cover, np.int64), np.asarray(nm, np.int32), np.asarray(mm, np.int32)


def finish_given(plan, primer_codes, ev):
    """host.Plan finished with given final primers (mp_plan_finish_given); plan.results() then returns them."""
    plan.finish_given(primer_codes, ev)
