"""ctypes binding of include/mprime.h.

The product loads `csrc/libmprime_hip.so` (hand-written HIP for gfx950) and fails loudly
when it is missing or cannot create a context on the GPU: there is no CPU fallback.
`Library(path)` accepts any library exporting the same C ABI; the test-suite uses that to
drive the host logic with the CPU oracle — the product never does.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

MP_MAX_K = 63
MP_NARROW_K = 31          # window words are uint32 up to here, uint64 above (mprime.h MP_WORD_BYTES)


def word_dtype(k: int):
    """numpy dtype of the window words of primer length k."""
    return np.uint32 if k <= MP_NARROW_K else np.uint64
MP_WIN_SKIP = 0x80000000
MP_ERR_CAPACITY = -4
MP_ERR_SHORT_WINDOW = -5

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB = os.path.join(HERE, "csrc", "libmprime_hip.so")

# every symbol include/mprime.h declares: (name, restype, argtypes)
_p = C.c_void_p
SYMBOLS = [
    ("mp_create", C.c_int, [C.c_int, C.POINTER(_p)]),
    ("mp_destroy", None, [_p]),
    ("mp_last_error", C.c_char_p, [_p]),
    ("mp_backend_name", C.c_char_p, []),
    ("mp_set_stream", C.c_int, [_p, _p]),
    ("mp_reserve_columns", C.c_int, [_p, C.c_int32]),
    ("mp_load_msa", C.c_int, [_p, _p, _p, C.c_int32]),
    ("mp_row_attributes", C.c_int, [_p, _p, _p, _p]),
    ("mp_row_histograms", C.c_int, [_p, C.c_int32, _p, _p]),
    ("mp_build_windows", C.c_int, [_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    ("mp_get_exceptions", C.c_int, [_p, C.c_int32, _p, _p, _p]),
    ("mp_set_extra_rows", C.c_int, [_p, C.c_int32, _p, _p]),
    ("mp_get_window_words", C.c_int, [_p, C.c_int32, C.c_int32, C.c_int32, _p]),
    ("mp_window_stats", C.c_int, [_p, _p, _p]),
    ("mp_window_unique", C.c_int, [_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    ("mp_set_entropy_gate", C.c_int, [_p, C.c_double]),
    ("mp_entropy_gate_result", C.c_int, [_p, C.POINTER(C.c_int32), _p]),
    ("mp_get_unique", C.c_int, [_p, _p, _p, _p, _p]),
    ("mp_get_labels", C.c_int, [_p, C.c_int32, _p]),
    ("mp_get_labels_many", C.c_int, [_p, C.c_int32, _p, _p]),
    ("mp_eval_candidates", C.c_int, [_p, C.c_int32, _p, _p, C.c_uint64, C.c_uint64, _p]),
    ("mp_eval_masks", C.c_int, [_p, C.c_int32, _p, _p, C.c_uint64, C.c_uint64, _p, _p]),
    ("mp_eval_masks_resident", C.c_int, [_p, C.c_int32, _p, _p, C.c_uint64, C.c_uint64]),
    ("mp_masks_set_bits", C.c_int, [_p, C.c_int64, _p, _p, _p, _p]),
    ("mp_masks_fetch", C.c_int, [_p, _p, _p]),
    ("mp_pair_coverage_resident", C.c_int, [_p, C.c_int64, _p, _p]),
    ("mp_eval_upload", C.c_int, [_p, C.c_int32, _p, _p, C.c_uint64, C.c_uint64]),
    ("mp_eval_launch", C.c_int, [_p, _p]),
    ("mp_eval_launch_rotating", C.c_int, [_p, _p, _p]),
    ("mp_window_stats_begin", C.c_int, [_p]),
    ("mp_window_stats_end", C.c_int, [_p, _p, _p]),
    ("mp_eval_launch_alt", C.c_int, [_p, _p]),
    ("mp_eval_sync", C.c_int, [_p]),
    ("mp_eval_timing", C.c_int, [_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    ("mp_eval_timing_samples", C.c_int, [_p, C.c_int32, _p, C.POINTER(C.c_int32)]),
    ("mp_eval_plan_info", C.c_int, [_p, _p]),
    ("mp_dimer_scan", C.c_int, [_p, C.c_int32, _p, _p, C.c_int32, C.c_int32, _p, _p, C.c_double, C.c_int64, _p,
                                C.POINTER(C.c_int64)]),
    ("mp_dimer_pairs", C.c_int, [_p, C.c_int32, _p, _p, C.c_int64, _p, _p, _p, C.c_double, _p]),
    ("mp_pair_coverage", C.c_int, [_p, C.c_int32, C.c_int32, _p, _p, C.c_int64, _p, _p]),
    ("mp_pcr_scan", C.c_int, [_p, _p, _p, C.c_int32, C.c_int32, _p, _p, _p]),
    ("mp_kmm_scan", C.c_int, [_p, _p, _p, C.c_int32, C.c_int32, _p, _p, C.c_int32, C.c_int32, C.c_int64, _p, C.POINTER(C.c_int64)]),
    ("mp_seq_load", C.c_int, [_p, _p, _p, C.c_int32]),
    ("mp_seq_free", C.c_int, [_p]),
    ("mp_seq_info", C.c_int, [_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("mp_pcr_scan_resident", C.c_int, [_p, C.c_int32, _p, _p, _p]),
    ("mp_kmm_scan_resident", C.c_int, [_p, C.c_int32, _p, _p, C.c_int32, C.c_int32, C.c_int64, _p, C.POINTER(C.c_int64)]),
    ("mp_comm_unique_id", C.c_int, [_p]),
    ("mp_comm_init", C.c_int, [_p, C.c_int32, C.c_int32, _p]),
    ("mp_comm_destroy", C.c_int, [_p]),
    ("mp_comm_describe", C.c_int, [_p, _p, C.c_char_p, C.c_int32]),
    ("mp_comm_allreduce_i64", C.c_int, [_p, _p, C.c_int64]),
    ("mp_comm_allreduce_host_i64", C.c_int, [_p, _p, C.c_int64]),
    ("mp_comm_allgather_i64", C.c_int, [_p, C.c_int64, _p]),
    ("mp_comm_allgatherv", C.c_int, [_p, _p, C.c_int64, _p, _p]),
    ("mp_comm_alltoall_counts", C.c_int, [_p, _p, _p]),
    ("mp_comm_alltoallv", C.c_int, [_p, _p, _p, _p, _p]),
    ("mp_eval_candidates_allreduce", C.c_int, [_p, C.c_int32, _p, _p, C.c_uint64, C.c_uint64, _p]),
    ("mp_device_bytes", C.c_int, [_p, C.POINTER(C.c_int64)]),
]
COMM_ID_BYTES = 128
# include/mprime_offtarget.h: the off-target screen on the device (csrc/offtarget.hip) — exported by libmprime_hip.so only; bound where
# a library has them (the oracle serves mprime.h alone: the checker of these calls is the host path of validate.py)
OFFTARGET_SYMBOLS = [
    ("mp_offtarget_resident", C.c_int, [_p, C.c_int32, _p, _p, _p, _p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _p, C.POINTER(C.c_int64)]),
    ("mp_amplicon_join", C.c_int, [_p, C.c_int64, _p, C.c_int32, C.c_int32, C.c_int64, _p, C.POINTER(C.c_int64)]),
    ("mp_offtarget_stats", C.c_int, [_p, _p, _p]),
]
# the gapped rule of the same header (csrc/kmm.hpp: kmm_gap_kernel): bound the same way; a library without them (the oracle) leaves
# validate.py to its host form of the rule
GAP_SYMBOLS = [
    ("mp_kmm_gap_scan_resident", C.c_int, [_p, C.c_int32, _p, _p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _p, C.POINTER(C.c_int64)]),
    ("mp_offtarget_gap_resident", C.c_int, [_p, C.c_int32, _p, _p, _p, _p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _p,
                                            C.POINTER(C.c_int64)]),
]
KMM_MAX_GAP = 4                     # MP_KMM_MAX_GAP


class AnchorParams(C.Structure):
    """mp_anchor_params (include/mprime_anchor.h)."""
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("band", C.c_int32),
                ("min_identity_permille", C.c_int32)]


# include/mprime_anchor.h: anchored alignment on the device (csrc/anchor.hip) — exported by libmprime_hip.so only and bound where a library
# has them; the checker of these calls is the plain restatement of the rule in tests/anchor_ref.py
ANCHOR_SYMBOLS = [
    ("mp_anchor_set", C.c_int, [_p, _p, C.c_int32, _p, C.c_int32, C.POINTER(AnchorParams)]),
    ("mp_anchor_align", C.c_int, [_p, C.c_int32, _p, _p, C.c_int32, _p, _p, _p, _p]),
    ("mp_anchor_stats", C.c_int, [_p, _p, _p]),
]
ANCHOR_REVERSED = 8                 # MP_ANCHOR_REVERSED
ANCHOR_MAX_LEN = 32767              # MP_ANCHOR_MAX_LEN
ANCHOR_MAX_BAND = 255               # MP_ANCHOR_MAX_BAND
ANCHOR_MAX_PARAM = 4095             # MP_ANCHOR_MAX_PARAM
ANCHOR_META = 10                    # MP_ANCHOR_META


class ClusterParams(C.Structure):
    """mp_cluster_params (include/mprime_cluster.h)."""
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("band", C.c_int32),
                ("identity_permille", C.c_int32), ("min_votes", C.c_int32)]


# include/mprime_cluster.h: clustering by identity on the device (csrc/cluster.hip) — exported by libmprime_hip.so only; the checker of
# these calls is the plain restatement of the rule in tests/cluster_ref.py
CLUSTER_SYMBOLS = [
    ("mp_cluster_load", C.c_int, [_p, C.c_int32, _p, _p]),
    ("mp_cluster_pairs", C.c_int, [_p, C.c_int64, _p, _p, C.POINTER(ClusterParams), _p]),
    ("mp_cluster_greedy", C.c_int, [_p, C.POINTER(ClusterParams), _p, _p, _p, C.POINTER(C.c_int32)]),
    ("mp_cluster_stats", C.c_int, [_p, _p, _p]),
]
CLUSTER_PAIR = 5                    # MP_CLUSTER_PAIR
# both strands: mp_anchor_strands (read by mp_anchor_align and mp_star_round), the both-strand clustering calls
STRAND_SYMBOLS = [
    ("mp_anchor_strands", C.c_int, [_p, C.c_int32]),
    ("mp_cluster_pairs_strands", C.c_int, [_p, C.c_int64, _p, _p, _p, C.POINTER(ClusterParams), _p]),
    ("mp_cluster_greedy_strands", C.c_int, [_p, C.POINTER(ClusterParams), _p, _p, _p, _p, C.POINTER(C.c_int32)]),
]

# include/mprime_star.h: the star alignment on the device (csrc/star.hip) — exported by libmprime_hip.so only; the checker of these calls
# is the plain restatement of the rule in tests/star_ref.py
STAR_SYMBOLS = [
    ("mp_star_load", C.c_int, [_p, C.c_int32, _p, _p]),
    ("mp_star_round", C.c_int, [_p, _p, C.c_int32, C.POINTER(AnchorParams), _p, _p, C.POINTER(C.c_int32)]),
    ("mp_star_rows", C.c_int, [_p, _p]),
    ("mp_star_counts", C.c_int, [_p, _p]),
    ("mp_star_stats", C.c_int, [_p, _p, _p]),
    ("mp_star_free", C.c_int, [_p]),
]
STAR_MAX_ROUNDS = 8                 # MP_STAR_MAX_ROUNDS
STAR_META = ANCHOR_META + 1         # MP_STAR_META
STAR_COUNTS = 6                     # MP_STAR_COUNTS

# include/mprime_ani.h: sketches and their comparison per pair of groups on the device (csrc/ani.hip) — exported by libmprime_hip.so only;
# the checker of these calls is the plain restatement of the rule in tests/ani_ref.py
ANI_SYMBOLS = [
    ("mp_ani_sketch", C.c_int, [_p, C.c_int32, _p, _p, C.c_int32]),
    ("mp_ani_sketches", C.c_int, [_p, _p, _p]),
    ("mp_ani_pairs", C.c_int, [_p, C.c_int64, _p, _p, _p]),
    ("mp_ani_groups", C.c_int, [_p, C.c_int32, _p, C.c_int64, _p, _p, C.c_int32, _p]),
    ("mp_ani_table", C.c_int, [_p]),
    ("mp_ani_stats", C.c_int, [_p, _p, _p]),
]
# both strands of include/mprime_ani.h: canonical sketches with orientation bits and the (same, opp) vote; the checker is
# tests/ani_strand_ref.py
ANI_STRAND_SYMBOLS = [
    ("mp_ani_sketch_strands", C.c_int, [_p, C.c_int32, _p, _p, C.c_int32]),
    ("mp_ani_orientations", C.c_int, [_p, _p]),
    ("mp_ani_pairs_strand", C.c_int, [_p, C.c_int64, _p, _p, _p]),
    ("mp_ani_groups_strand", C.c_int, [_p, C.c_int32, _p, C.c_int64, _p, _p, C.c_int32, _p]),
]
ANI_MIN_SKETCH = 16                 # MP_ANI_MIN_SKETCH
ANI_MAX_SKETCH = 1024               # MP_ANI_MAX_SKETCH
ANI_TABLE = 1025                    # MP_ANI_TABLE
ANI_PAIR = 3                        # MP_ANI_PAIR
ANI_PPM = 1000000                   # MP_ANI_PPM
# include/mprime_dege.h: DegePrime's degenerate oligomer per window on the device (csrc/dege.hip) — exported by libmprime_hip.so only; the
# checker of these calls is the plain restatement of the rule in tests/dege_ref.py
DEGE_SYMBOLS = [
    ("mp_dege_load", C.c_int, [_p, C.c_int32, C.c_int32, _p]),
    ("mp_dege_windows", C.c_int, [_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    ("mp_dege_window_table", C.c_int, [_p, _p, _p]),
    ("mp_dege_unique", C.c_int, [_p, C.c_int32, C.c_int64, _p, _p]),
    ("mp_dege_merge", C.c_int, [_p, C.c_int32, C.c_int32, C.c_uint64]),
    ("mp_dege_best", C.c_int, [_p, _p]),
    ("mp_dege_iterations", C.c_int, [_p, C.c_int32, _p]),
    ("mp_dege_stats", C.c_int, [_p, _p, _p]),
]
DEGE_MIN_L, DEGE_MAX_L = 2, 32      # MP_DEGE_MIN_L, MP_DEGE_MAX_L
DEGE_MAX_DRAWS = 100                # MP_DEGE_MAX_DRAWS
DEGE_MAX_ITERS = 65536              # MP_DEGE_MAX_ITERS
DEGE_LDS_SLOTS = 4096               # MP_DEGE_LDS_SLOTS
DEGE_LDS_LIMIT = 3072               # MP_DEGE_LDS_LIMIT: more distinct mers in a window take the global-memory table
DEGE_SORT_MIN = 64                  # MP_DEGE_SORT_MIN: the sort sizes are the powers of two from here
DEGE_MERGE_LDS = 4096               # MP_DEGE_MERGE_LDS: more unique mers in a window are merged from global memory
DEGE_WIN = 4                        # MP_DEGE_WIN
DEGE_REC = 35                       # MP_DEGE_REC
# include/mprime_ont.h: read ends against expanded primers on the device (csrc/ont.hip) — exported by libmprime_hip.so only; the checker of
# these calls is difflib itself beside the plain restatement of the rule in tests/ont_ref.py
ONT_SYMBOLS = [
    ("mp_ont_set_keys", C.c_int, [_p, C.c_int32, _p, _p]),
    ("mp_ont_assign", C.c_int, [_p, C.c_int64, _p, _p, _p, _p, _p]),
    ("mp_ont_stats", C.c_int, [_p, _p, _p]),
]
ONT_MAX_LEN = 64                    # MP_ONT_MAX_LEN
# include/mprime_panel.h: the panel update (cross-set dimer search in csrc/dimer.hip, class joins in csrc/offtarget.hip) — exported by
# libmprime_hip.so only; the checker of these calls is the plain restatement of the rule in tests/panel_ref.py
PANEL_SYMBOLS = [
    ("mp_dimer_cross", C.c_int, [_p, C.c_int32, _p, _p, C.c_int32, _p, _p, _p, C.c_double, C.c_int64, _p, C.POINTER(C.c_int64)]),
    ("mp_amplicon_join_classes", C.c_int, [_p, C.c_int64, _p, C.c_int32, C.c_int32, C.c_int64, _p, C.POINTER(C.c_int64)]),
    ("mp_offtarget_classes", C.c_int, [_p, C.c_int32, _p, _p, _p, _p, _p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _p, C.POINTER(C.c_int64)]),
]
ONT_Q_ROWS, ONT_Q_COLS = 129, 65    # MP_ONT_Q_ROWS, MP_ONT_Q_COLS
# include/mprime_setscreen.h: per-pair product counts for the off-target-aware set cover (csrc/setscreen.hip) — exported by
# libmprime_hip.so only; the checker of these calls is the plain restatement of the rule in tests/setscreen_ref.py
SETSCREEN_SYMBOLS = [
    ("mp_setscreen_begin", C.c_int, [_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ("mp_setscreen_add", C.c_int, [_p, C.c_int32, _p, _p, _p, C.c_int64, _p, C.POINTER(C.c_int64)]),
    ("mp_setscreen_site_counts", C.c_int, [_p, C.c_int32, C.c_int32, _p, _p]),
    ("mp_setscreen_stats", C.c_int, [_p, _p, _p]),
    ("mp_setscreen_end", C.c_int, [_p]),
    ("mp_setscreen_join", C.c_int, [_p, C.c_int64, _p, C.c_int32, C.c_int32, C.c_int64, _p, C.POINTER(C.c_int64)]),
]
SETSCREEN_BIN = 1024                # MP_SETSCREEN_BIN


def prefer_staged_copies():
    """For the drop-in command lines, called before anything starts the HIP runtime: read-backs into ordinary numpy arrays go
    through the runtime's staging buffers instead of page-locking the array for one use (GPU_PINNED_MIN_XFER_SIZE = 256 MiB: the
    58 MB of histogram entries of a 131072 x 1000 alignment take 6.5 ms instead of 27-32 ms, csrc/api.hip).  A process-wide runtime
    setting, hence a decision of the PROGRAM, not of the library: the class API leaves it alone.  A value the user exported, or
    MP_KEEP_PIN_THRESHOLD, wins."""
    if not os.environ.get("MP_KEEP_PIN_THRESHOLD"):
        os.environ.setdefault("GPU_PINNED_MIN_XFER_SIZE", "256")


def one_hip_runtime():
    """One HIP runtime per process.  torch ships its own libamdhip64 / libhsa-runtime64 (torch/lib); libmprime_hip.so is linked against
    the system's (/opt/rocm).  The file names differ but the SONAMEs agree, so whichever is loaded FIRST serves both — and when this
    library comes first and torch second, the loader finds torch's copy by its run path and the process ends up with two HIP and two
    HSA runtimes on one GPU: torch then reports "No HIP GPUs are available" (tools/maps_check.py), and what else two runtimes do to
    each other's registered memory is anybody's guess (the unexplained SIGABRT of round 4 is a candidate).  So before
    the HIP library is opened in a process where torch is installed but not imported yet, torch's runtime is opened first — exactly the
    state of a process that imported torch first (bench.py, the GPU suite).  MP_KEEP_SYSTEM_HIP=1 leaves the order to the caller."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("MP_KEEP_SYSTEM_HIP") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    loaded = []
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                loaded.append((name, C.CDLL(path, mode=C.RTLD_GLOBAL)))
            except OSError as e:
                # [r6, advisor] a half-loaded pair (torch's HSA, the system's HIP) is the mixed state this function exists to prevent
                if loaded:
                    raise MprimeError(-2, f"torch's {loaded[0][0]} is loaded but its {name} is not ({e}): refusing to run on a mixed pair of HIP "
                                          "runtimes (MP_KEEP_SYSTEM_HIP=1 skips this step)") from None
                return
    # the runtime that now serves the process against the one libmprime_hip.so was built with (hipcc of /opt/rocm): a different MAJOR is refused
    if len(loaded) == 2:
        ver = C.c_int(0)
        try:
            if loaded[1][1].hipRuntimeGetVersion(C.byref(ver)) == 0:
                major = ver.value // 10000000
                built = int(os.environ.get("MP_BUILT_HIP_MAJOR", "7"))
                if os.environ.get("MP_TRACE"):
                    print(f"[mprime] HIP runtime bound: torch's ({libdir}), version {ver.value}; library built with HIP {built}.x", file=sys.stderr)
                if major != built:
                    raise MprimeError(-2, f"torch's HIP runtime is version {ver.value} (major {major}), libmprime_hip.so was built with HIP {built}.x: "
                                          "set MP_KEEP_SYSTEM_HIP=1 to run on the system's runtime instead")
        except AttributeError:
            pass


class MprimeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mprime error {code}: {msg}")
        self.code = code


class Library:
    """A shared library exporting the mprime C ABI."""

    def __init__(self, path: str | None = None):
        # Without an explicit path the library IS the product's backend: libmprime_hip.so, or another BUILD of it named by
        # MPRIME_LIBRARY (a debug / sanitizer build).  Whatever it is, it must say mp_backend_name() == "hip": no environment variable
        # can put the ABI checker behind a drop-in command (the CPU-only CLI tests patch this class from tests/checker_shim/).
        # Library(path) — what tests and tools do — loads what it is told to.
        implicit = path is None
        path = path or os.environ.get("MPRIME_LIBRARY") or HIP_LIB
        if not os.path.exists(path):
            raise MprimeError(-2, f"{path} is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                  "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        self.path = path
        if os.path.basename(path).startswith("libmprime_hip"):
            one_hip_runtime()
        self.dll = C.CDLL(path)
        for name, res, args in SYMBOLS:
            fn = getattr(self.dll, name)     # AttributeError = ABI symbol missing
            fn.restype = res
            fn.argtypes = args
        self.backend = self.dll.mp_backend_name().decode()
        self.offtarget = all(hasattr(self.dll, name) for name, _, _ in OFFTARGET_SYMBOLS)
        if self.backend == "hip" and not self.offtarget:
            raise MprimeError(-2, f"{path} lacks the off-target entry points of include/mprime_offtarget.h: rebuild it")
        self.gapscan = all(hasattr(self.dll, name) for name, _, _ in GAP_SYMBOLS)
        if self.backend == "hip" and not self.gapscan:
            raise MprimeError(-2, f"{path} lacks the gapped-scan entry points of include/mprime_offtarget.h: rebuild it")
        self.anchor = all(hasattr(self.dll, name) for name, _, _ in ANCHOR_SYMBOLS)
        if self.backend == "hip" and not self.anchor:
            raise MprimeError(-2, f"{path} lacks the anchored-alignment entry points of include/mprime_anchor.h: rebuild it")
        self.cluster = all(hasattr(self.dll, name) for name, _, _ in CLUSTER_SYMBOLS)
        if self.backend == "hip" and not self.cluster:
            raise MprimeError(-2, f"{path} lacks the clustering entry points of include/mprime_cluster.h: rebuild it")
        self.star = all(hasattr(self.dll, name) for name, _, _ in STAR_SYMBOLS)
        if self.backend == "hip" and not self.star:
            raise MprimeError(-2, f"{path} lacks the star-alignment entry points of include/mprime_star.h: rebuild it")
        self.strands = all(hasattr(self.dll, name) for name, _, _ in STRAND_SYMBOLS)
        if self.backend == "hip" and not self.strands:
            raise MprimeError(-2, f"{path} lacks the both-strand entry points of include/mprime_anchor.h and include/mprime_cluster.h: rebuild it")
        self.ani = all(hasattr(self.dll, name) for name, _, _ in ANI_SYMBOLS)
        if self.backend == "hip" and not self.ani:
            raise MprimeError(-2, f"{path} lacks the identity-merge entry points of include/mprime_ani.h: rebuild it")
        self.ani_strands = all(hasattr(self.dll, name) for name, _, _ in ANI_STRAND_SYMBOLS)
        if self.backend == "hip" and not self.ani_strands:
            raise MprimeError(-2, f"{path} lacks the both-strand entry points of include/mprime_ani.h: rebuild it")
        self.dege = all(hasattr(self.dll, name) for name, _, _ in DEGE_SYMBOLS)
        if self.backend == "hip" and not self.dege:
            raise MprimeError(-2, f"{path} lacks the DegePrime entry points of include/mprime_dege.h: rebuild it")
        self.ont = all(hasattr(self.dll, name) for name, _, _ in ONT_SYMBOLS)
        if self.backend == "hip" and not self.ont:
            raise MprimeError(-2, f"{path} lacks the read-assignment entry points of include/mprime_ont.h: rebuild it")
        self.panel = all(hasattr(self.dll, name) for name, _, _ in PANEL_SYMBOLS)
        if self.backend == "hip" and not self.panel:
            raise MprimeError(-2, f"{path} lacks the panel-update entry points of include/mprime_panel.h: rebuild it")
        self.setscreen = all(hasattr(self.dll, name) for name, _, _ in SETSCREEN_SYMBOLS)
        if self.backend == "hip" and not self.setscreen:
            raise MprimeError(-2, f"{path} lacks the set-screen entry points of include/mprime_setscreen.h: rebuild it")
        for name, res, args in ((PANEL_SYMBOLS if self.panel else []) + (SETSCREEN_SYMBOLS if self.setscreen else []) + (OFFTARGET_SYMBOLS if self.offtarget else []) + (GAP_SYMBOLS if self.gapscan else []) +
                                (ANCHOR_SYMBOLS if self.anchor else []) + (CLUSTER_SYMBOLS if self.cluster else []) +
                                (STAR_SYMBOLS if self.star else []) + (ANI_SYMBOLS if self.ani else []) +
                                (DEGE_SYMBOLS if self.dege else []) + (ONT_SYMBOLS if self.ont else []) +
                                (STRAND_SYMBOLS if self.strands else []) + (ANI_STRAND_SYMBOLS if self.ani_strands else [])):
            fn = getattr(self.dll, name)
            fn.restype = res
            fn.argtypes = args
        if implicit and self.backend != "hip":
            raise MprimeError(-2, f"{path} reports backend {self.backend!r}, not 'hip': the product runs on libmprime_hip.so only "
                                  "(MPRIME_LIBRARY may name another build of it, not the CPU checker)")

    def context(self, device: int = 0) -> "Context":
        return Context(self, device)

    def ani_table(self) -> np.ndarray:
        """int32 [ANI_TABLE]: TAB of include/mprime_ani.h (mp_ani_table; needs no device)."""
        if not self.ani:
            raise MprimeError(-2, f"{self.path} does not serve include/mprime_ani.h (libmprime_hip.so does)")
        out = np.zeros(ANI_TABLE, np.int32)
        rc = self.dll.mp_ani_table(_ptr(out))
        if rc != 0:
            raise MprimeError(rc, "mp_ani_table")
        return out


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Context:
    """One opaque mp_ctx (one GPU)."""

    def __init__(self, lib: Library, device: int = 0):
        self.lib = lib
        self.d = lib.dll
        h = C.c_void_p()
        rc = self.d.mp_create(device, C.byref(h))
        if rc != 0:
            msg = self.d.mp_last_error(h).decode() if h else "mp_create failed (no usable GPU?)"
            raise MprimeError(rc, msg)
        self.h = h
        self.n_rows = 0
        self.n_win = 0
        self.k = 0

    def close(self):
        if self.h:
            self.d.mp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise MprimeError(rc, self.d.mp_last_error(self.h).decode())

    def set_stream(self, stream_handle: int):
        self._ck(self.d.mp_set_stream(self.h, C.c_void_p(stream_handle)))

    # (1)
    def reserve_columns(self, n_columns: int):
        """Row shards: the alignment is at least this wide even if no local row is (call before load_msa)."""
        self._ck(self.d.mp_reserve_columns(self.h, int(n_columns)))

    def load_msa(self, data: np.ndarray, row_off: np.ndarray):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        self.n_rows = len(row_off) - 1
        self._ck(self.d.mp_load_msa(self.h, _ptr(data), _ptr(row_off), self.n_rows))

    def row_attributes(self):
        lead = np.empty(self.n_rows, np.int32)
        rstrip = np.empty(self.n_rows, np.int32)
        rlen = np.empty(self.n_rows, np.int32)
        self._ck(self.d.mp_row_attributes(self.h, _ptr(lead), _ptr(rstrip), _ptr(rlen)))
        return lead, rstrip, rlen

    def row_histograms(self, n_bins: int):
        """(lead_hist, rstrip_hist) int64 [n_bins]: rows per leading-gap length / per right-stripped length."""
        lead = np.empty(n_bins, np.int64)
        rstrip = np.empty(n_bins, np.int64)
        self._ck(self.d.mp_row_histograms(self.h, n_bins, _ptr(lead), _ptr(rstrip)))
        return lead, rstrip

    # (2)
    def build_windows(self, p0: int, n_windows: int, k: int, v: int) -> int:
        n_ex = C.c_int32(0)
        self._ck(self.d.mp_build_windows(self.h, p0, n_windows, k, v, C.byref(n_ex)))
        self.n_win, self.k = n_windows, k
        return n_ex.value

    def get_exceptions(self, n_ex: int):
        w = np.empty(max(n_ex, 1), np.int32)
        r = np.empty(max(n_ex, 1), np.int32)
        codes = np.empty((max(n_ex, 1), self.k), np.uint8)
        self._ck(self.d.mp_get_exceptions(self.h, max(n_ex, 1), _ptr(w), _ptr(r), _ptr(codes)))
        return w[:n_ex], r[:n_ex], codes[:n_ex]

    def set_extra_rows(self, window: np.ndarray, words: np.ndarray):
        window = np.ascontiguousarray(window, dtype=np.int32)
        words = np.ascontiguousarray(words, dtype=word_dtype(self.k)).reshape(-1, 3)
        self._ck(self.d.mp_set_extra_rows(self.h, len(window), _ptr(window), _ptr(words)))

    def get_window_words(self, w: int, row0: int = 0, n: int | None = None) -> np.ndarray:
        n = self.n_rows - row0 if n is None else n
        out = np.empty((3, n), word_dtype(self.k))
        self._ck(self.d.mp_get_window_words(self.h, w, row0, n, _ptr(out)))
        return out

    # (3)
    def window_unique(self, want_labels: bool = False, cap_entries: int | None = None, sort: bool = True):
        """Returns (win_off[W+1], words[3][n], count[n], first_row[n]).  sort=True: the entries of every window sorted
        by first_row (the ABI leaves the order unspecified) plus the permutation needed to translate device labels;
        sort=False: as the library returned them (the native planning stage orders them itself)."""
        cap = cap_entries or max(1 << 16, min(self.n_rows * self.n_win, 1 << 24))
        n = C.c_int64(0)
        rc = self.d.mp_window_unique(self.h, cap, int(want_labels), C.byref(n))
        if rc == MP_ERR_CAPACITY:
            cap = int(n.value)
            rc = self.d.mp_window_unique(self.h, cap, int(want_labels), C.byref(n))
        self._ck(rc)
        n = int(n.value)
        off = np.empty(self.n_win + 1, np.int64)
        count = np.empty(max(n, 1), np.int32)
        first = np.empty(max(n, 1), np.int32)
        # the C side packs words as [3][n]; allocate exactly so the strides agree
        wbuf = np.empty(3 * max(n, 1), word_dtype(self.k))
        self._ck(self.d.mp_get_unique(self.h, _ptr(off), _ptr(wbuf), _ptr(count), _ptr(first)))
        words = wbuf[:3 * n].reshape(3, n) if n else np.zeros((3, 0), word_dtype(self.k))
        count, first = count[:n], first[:n]
        self._off = off
        if not sort:
            self._label_rank = None
            return off, words, count, first
        win_of = np.repeat(np.arange(self.n_win), np.diff(off))
        order = np.argsort((win_of.astype(np.int64) << 32) | first.astype(np.int64))     # (window, first row): all distinct
        self._label_rank = np.empty(n, np.int64)          # device index -> index within window, first-seen order
        self._label_rank[order] = np.arange(n) - off[win_of[order]]
        self._off = off
        return off, words[:, order], count[order], first[order]

    def window_unique_device(self, cap_entries: int | None = None) -> int:
        """The histograms only (mp_window_unique without labels): the entries stay on the device for host.Plan(device_context=...),
        which reads them back beside the planning.  Returns their number."""
        cap = cap_entries or max(1 << 16, min(self.n_rows * self.n_win, 1 << 24))
        n = C.c_int64(0)
        rc = self.d.mp_window_unique(self.h, cap, 0, C.byref(n))
        if rc == MP_ERR_CAPACITY:
            rc = self.d.mp_window_unique(self.h, int(n.value), 0, C.byref(n))
        self._ck(rc)
        return int(n.value)

    def set_entropy_gate(self, threshold: float):
        """Arm (threshold > 0) or disarm (0) the entropy gate on the device for the following window_unique_device calls."""
        self._ck(self.d.mp_set_entropy_gate(self.h, float(threshold)))

    def entropy_gate_result(self):
        """(number of windows the last histogram call rejected on the device, bool [n_win] which)."""
        n = C.c_int32(0)
        which = np.zeros(max(self.n_win, 1), np.uint8)
        self._ck(self.d.mp_entropy_gate_result(self.h, C.byref(n), _ptr(which)))
        return int(n.value), which[: self.n_win].astype(bool)

    def get_labels(self, w: int) -> np.ndarray:
        lab = np.empty(self.n_rows, np.int32)
        self._ck(self.d.mp_get_labels(self.h, w, _ptr(lab)))
        out = np.full(self.n_rows, -1, np.int64)
        ok = lab >= 0
        out[ok] = self._label_rank[self._off[w] + lab[ok]]
        return out

    def get_labels_raw(self, windows) -> np.ndarray:
        """[len(windows)][n_rows] int32: mp_get_labels of each window as the library returns them (index of the row's entry inside
        the window's segment of mp_get_unique, -1 = the row is not in the histogram)."""
        out = np.empty((max(len(windows), 1), self.n_rows), np.int32)
        wins = np.ascontiguousarray(windows, dtype=np.int32)
        self._ck(self.d.mp_get_labels_many(self.h, len(wins), _ptr(wins), _ptr(out)))
        return out[: len(windows)]

    # (4)
    def window_stats(self):
        """(freq [W][4][k], nn [W][k-1][4][4]) int64: per-window base counts and nearest-neighbour pair counts
        over the universe (state_matrix / trans_matrix, V20:541-577)."""
        freq = np.zeros((self.n_win, 4, self.k), np.int64)
        nn = np.zeros((self.n_win, self.k - 1, 4, 4), np.int64)
        self._ck(self.d.mp_window_stats(self.h, _ptr(freq), _ptr(nn)))
        return freq, nn

    def window_stats_begin(self):
        """window_stats in two halves (mp_window_stats_begin): the kernel and the read-back of its counters start on the context's second
        stream; returns the (freq, nn) arrays the counters will land in — valid after window_stats_end(freq, nn), or after a
        host.Plan(device_context=...) built with them (mp_plan_create_streamed ends a pending begin itself)."""
        freq = np.zeros((self.n_win, 4, self.k), np.int64)
        nn = np.zeros((self.n_win, self.k - 1, 4, 4), np.int64)
        self._ck(self.d.mp_window_stats_begin(self.h))
        return freq, nn

    def window_stats_end(self, freq, nn):
        self._ck(self.d.mp_window_stats_end(self.h, _ptr(freq), _ptr(nn)))

    def eval_candidates(self, cand_window, cand_codes, strictF: int, strictR: int) -> np.ndarray:
        cand_window = np.ascontiguousarray(cand_window, dtype=np.int32)
        cand_codes = np.ascontiguousarray(cand_codes, dtype=np.uint8).reshape(len(cand_window), self.k)
        out = np.zeros((len(cand_window), 3), np.int64)
        self._ck(self.d.mp_eval_candidates(self.h, len(cand_window), _ptr(cand_window), _ptr(cand_codes),
                                           strictF, strictR, _ptr(out)))
        return out

    # -- row shards (mprime.h section 9): RCCL behind the C ABI ---------------------------------------------------------------
    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        rc = self.d.mp_comm_unique_id(buf)
        if rc != 0:
            raise MprimeError(rc, "mp_comm_unique_id failed (librccl.so not loadable?)")
        return bytes(buf)

    def comm_init(self, n_ranks: int, rank: int, unique_id: bytes | None):
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id) if unique_id is not None else None
        self._ck(self.d.mp_comm_init(self.h, n_ranks, rank, buf))

    def comm_destroy(self):
        self._ck(self.d.mp_comm_destroy(self.h))

    def comm_describe(self):
        """(ranks the communicator reports, this rank as it reports it, path of the librccl in use or '')."""
        seen = np.zeros(2, np.int32)
        buf = C.create_string_buffer(512)
        self._ck(self.d.mp_comm_describe(self.h, _ptr(seen), buf, 512))
        return int(seen[0]), int(seen[1]), buf.value.decode()

    def comm_allreduce_device(self, device_ptr: int, n: int):
        self._ck(self.d.mp_comm_allreduce_i64(self.h, C.c_void_p(device_ptr), n))

    def comm_sum(self, a) -> np.ndarray:
        """Element-wise sum over the ranks of an int64 host array."""
        out = np.ascontiguousarray(a, dtype=np.int64).copy()
        self._ck(self.d.mp_comm_allreduce_host_i64(self.h, _ptr(out), out.size))
        return out

    def comm_gather_bytes(self, payload: np.ndarray, n_ranks: int):
        """(concatenation over ranks of a byte array whose length differs per rank, lengths per rank)."""
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        counts = np.zeros(n_ranks, np.int64)
        self._ck(self.d.mp_comm_allgather_i64(self.h, payload.size, _ptr(counts)))
        out = np.empty(int(counts.sum()), np.uint8)
        self._ck(self.d.mp_comm_allgatherv(self.h, _ptr(payload) if payload.size else None, payload.size, _ptr(counts),
                                           _ptr(out) if out.size else None))
        return out, counts

    def comm_exchange_bytes(self, payload: np.ndarray, send_counts):
        """Personalised exchange: `payload` holds send_counts[r] bytes for every rank r, in rank order.  Returns (the bytes this rank
        receives, source rank by source rank; their counts)."""
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        send_counts = np.ascontiguousarray(send_counts, dtype=np.int64)
        recv_counts = np.zeros(len(send_counts), np.int64)
        self._ck(self.d.mp_comm_alltoall_counts(self.h, _ptr(send_counts), _ptr(recv_counts)))
        out = np.empty(int(recv_counts.sum()), np.uint8)
        self._ck(self.d.mp_comm_alltoallv(self.h, _ptr(payload) if payload.size else None, _ptr(send_counts),
                                          _ptr(out) if out.size else None, _ptr(recv_counts)))
        return out, recv_counts

    def eval_candidates_allreduce(self, cand_window, cand_codes, strictF: int, strictR: int) -> np.ndarray:
        cand_window = np.ascontiguousarray(cand_window, dtype=np.int32)
        cand_codes = np.ascontiguousarray(cand_codes, dtype=np.uint8).reshape(len(cand_window), self.k)
        out = np.zeros((len(cand_window), 3), np.int64)
        self._ck(self.d.mp_eval_candidates_allreduce(self.h, len(cand_window), _ptr(cand_window), _ptr(cand_codes), strictF, strictR,
                                                     _ptr(out)))
        return out

    def eval_masks(self, cand_window, cand_codes, strictF: int, strictR: int):
        """(not_f, not_r): uint64 [n_cand][(n_rows+63)//64] — sequences a forward / reverse primer does not reach."""
        cand_window = np.ascontiguousarray(cand_window, dtype=np.int32)
        cand_codes = np.ascontiguousarray(cand_codes, dtype=np.uint8).reshape(len(cand_window), self.k)
        nw = (self.n_rows + 63) // 64
        nf = np.zeros((max(len(cand_window), 1), nw), np.uint64)
        nr = np.zeros((max(len(cand_window), 1), nw), np.uint64)
        self._ck(self.d.mp_eval_masks(self.h, len(cand_window), _ptr(cand_window), _ptr(cand_codes), strictF, strictR,
                                      _ptr(nf), _ptr(nr)))
        return nf[: len(cand_window)], nr[: len(cand_window)]

    def eval_masks_resident(self, cand_window, cand_codes, strictF: int, strictR: int):
        """The same masks, left in device memory (fetch with masks_fetch, combine with pair_coverage_resident)."""
        cand_window = np.ascontiguousarray(cand_window, dtype=np.int32)
        cand_codes = np.ascontiguousarray(cand_codes, dtype=np.uint8).reshape(len(cand_window), self.k)
        self._ck(self.d.mp_eval_masks_resident(self.h, len(cand_window), _ptr(cand_window), _ptr(cand_codes), strictF, strictR))
        self.n_masks = len(cand_window)

    def masks_set_bits(self, cand, row, which, value):
        cand = np.ascontiguousarray(cand, dtype=np.int32)
        row = np.ascontiguousarray(row, dtype=np.int32)
        which = np.ascontiguousarray(which, dtype=np.uint8)
        value = np.ascontiguousarray(value, dtype=np.uint8)
        self._ck(self.d.mp_masks_set_bits(self.h, len(cand), _ptr(cand), _ptr(row), _ptr(which), _ptr(value)))

    def masks_fetch(self):
        nw = (self.n_rows + 63) // 64
        nf = np.zeros((max(self.n_masks, 1), nw), np.uint64)
        nr = np.zeros((max(self.n_masks, 1), nw), np.uint64)
        if self.n_masks:
            self._ck(self.d.mp_masks_fetch(self.h, _ptr(nf), _ptr(nr)))
        return nf[: self.n_masks], nr[: self.n_masks]

    def pair_coverage_resident(self, pairs) -> np.ndarray:
        """popcount(not_f[i] | not_r[j]) over the resident masks for every (i, j) in pairs."""
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.zeros(max(len(pairs), 1), np.int32)
        self._ck(self.d.mp_pair_coverage_resident(self.h, len(pairs), _ptr(pairs), _ptr(out)))
        return out[: len(pairs)]

    def eval_upload(self, cand_window, cand_codes, strictF: int, strictR: int):
        cand_window = np.ascontiguousarray(cand_window, dtype=np.int32)
        cand_codes = np.ascontiguousarray(cand_codes, dtype=np.uint8).reshape(len(cand_window), self.k)
        self._ck(self.d.mp_eval_upload(self.h, len(cand_window), _ptr(cand_window), _ptr(cand_codes), strictF, strictR))

    def eval_launch(self, out_ptr: int):
        self._ck(self.d.mp_eval_launch(self.h, C.c_void_p(out_ptr)))

    def eval_launch_rotating(self, out_ptr: int, clear_ptr: int = 0):
        """Evaluate into the zeroed block at out_ptr; the same launch zeroes the block at clear_ptr (0: none) for the next one."""
        self._ck(self.d.mp_eval_launch_rotating(self.h, C.c_void_p(out_ptr), C.c_void_p(clear_ptr) if clear_ptr else None))

    def eval_launch_alt(self, out_ptr: int):
        """eval_launch on the context's second stream (mp_eval_launch_alt): alternate with eval_launch, different counter blocks."""
        self._ck(self.d.mp_eval_launch_alt(self.h, C.c_void_p(out_ptr)))

    def eval_sync(self):
        self._ck(self.d.mp_eval_sync(self.h))

    def eval_timing(self, reset: bool = False):
        ms, n = C.c_double(0), C.c_int32(0)
        self._ck(self.d.mp_eval_timing(self.h, int(reset), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def eval_plan_info(self) -> dict:
        """Which kernels the staged candidates go to (mp_eval_plan_info)."""
        info = np.zeros(4, np.int32)
        self._ck(self.d.mp_eval_plan_info(self.h, _ptr(info)))
        return {"chain_items": int(info[0]), "table_items": int(info[1]), "sliding_items": int(info[2]), "first_pass_chain_items": int(info[3])}

    def eval_timing_samples(self) -> np.ndarray:
        """Durations (ms) of the timed launches behind the last eval_timing() call."""
        n = C.c_int32(0)
        buf = np.zeros(4096, np.float32)
        self._ck(self.d.mp_eval_timing_samples(self.h, 4096, _ptr(buf), C.byref(n)))
        return buf[: min(n.value, 4096)].copy()

    # (5)
    def dimer_scan(self, codes: np.ndarray, off: np.ndarray, mode: int, n_new: int, loss_hit: np.ndarray,
                   dg_params: np.ndarray, dg_limit: float, cap: int = 1 << 16) -> np.ndarray:
        """Hit records [n][6] = (x, y, end length, end expansion, y expansion, idx), sorted."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int32)
        loss_hit = np.ascontiguousarray(loss_hit, dtype=np.uint8)
        dg_params = np.ascontiguousarray(dg_params, dtype=np.float64)
        while True:
            hits = np.empty((max(cap, 1), 6), np.int32)
            n = C.c_int64(0)
            self._ck(self.d.mp_dimer_scan(self.h, len(off) - 1, _ptr(codes), _ptr(off), mode, n_new, _ptr(loss_hit),
                                          _ptr(dg_params), dg_limit, cap, _ptr(hits), C.byref(n)))
            if n.value <= cap:
                h = hits[: n.value]
                return h[np.lexsort((h[:, 1], h[:, 0]))] if len(h) else h
            cap = int(n.value)

    def dimer_any(self, codes, off, mode: int, n_new: int, loss_hit, dg_params, dg_limit: float) -> bool:
        """True iff the scan has at least one hit (no hit records fetched, no re-scan with a larger buffer)."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int32)
        loss_hit = np.ascontiguousarray(loss_hit, dtype=np.uint8)
        dg_params = np.ascontiguousarray(dg_params, dtype=np.float64)
        n = C.c_int64(0)
        self._ck(self.d.mp_dimer_scan(self.h, len(off) - 1, _ptr(codes), _ptr(off), mode, n_new, _ptr(loss_hit), _ptr(dg_params),
                                      dg_limit, 0, None, C.byref(n)))
        return n.value > 0

    def dimer_pairs(self, codes, off, pairs, loss_hit, dg_params, dg_limit: float) -> np.ndarray:
        """flags[p] = 1 if the ordered pair (pairs[p,0] -> pairs[p,1]) forms a 3'-end dimer."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int32)
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        loss_hit = np.ascontiguousarray(loss_hit, dtype=np.uint8)
        dg_params = np.ascontiguousarray(dg_params, dtype=np.float64)
        flags = np.zeros(max(len(pairs), 1), np.uint8)
        self._ck(self.d.mp_dimer_pairs(self.h, len(off) - 1, _ptr(codes), _ptr(off), len(pairs), _ptr(pairs), _ptr(loss_hit),
                                       _ptr(dg_params), dg_limit, _ptr(flags)))
        return flags[: len(pairs)]

    def pair_coverage(self, sets_a, sets_b, pairs) -> np.ndarray:
        """popcount(sets_a[i] | sets_b[j]) for every (i, j) in pairs; sets are rows of uint64 words."""
        sets_a = np.ascontiguousarray(sets_a, dtype=np.uint64)
        sets_b = np.ascontiguousarray(sets_b, dtype=np.uint64)
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        out = np.zeros(max(len(pairs), 1), np.int32)
        self._ck(self.d.mp_pair_coverage(self.h, sets_a.shape[0], sets_a.shape[1], _ptr(sets_a), _ptr(sets_b), len(pairs),
                                         _ptr(pairs), _ptr(out)))
        return out[: len(pairs)]

    def pcr_scan(self, data, row_off, codes, off) -> np.ndarray:
        """[n_pairs][n_rows][4] = (forward expansion, amplicon start, reverse expansion, position of RC(reverse)); -1 = none."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int32)
        n_rows, n_pairs = len(row_off) - 1, (len(off) - 1) // 2
        out = np.full((max(n_pairs, 1), max(n_rows, 1), 4), -1, np.int32)
        self._ck(self.d.mp_pcr_scan(self.h, _ptr(data), _ptr(row_off), n_rows, n_pairs, _ptr(codes), _ptr(off), _ptr(out)))
        return out[:n_pairs, :n_rows]

    def kmm_scan(self, data, row_off, pat_codes, pat_off, max_mismatch: int, term: int, cap: int = 1 << 20) -> np.ndarray:
        """Hits [n][4] = (sequence, start, pattern, strand) of the k-mismatch primer-site scan, sorted."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        pat_codes = np.ascontiguousarray(pat_codes, dtype=np.uint8)
        pat_off = np.ascontiguousarray(pat_off, dtype=np.int32)
        while True:
            hits = np.empty((max(cap, 1), 4), np.int32)
            n = C.c_int64(0)
            self._ck(self.d.mp_kmm_scan(self.h, _ptr(data), _ptr(row_off), len(row_off) - 1, len(pat_off) - 1, _ptr(pat_codes),
                                        _ptr(pat_off), int(max_mismatch), int(term), cap, _ptr(hits), C.byref(n)))
            if n.value <= cap:
                h = hits[: n.value]
                return h[np.lexsort((h[:, 3], h[:, 2], h[:, 1], h[:, 0]))] if len(h) else h
            cap = int(n.value)

    # (8b) the resident sequence store
    def seq_load(self, data, row_off):
        """The unaligned database of the PCR / k-mismatch scans, uploaded and packed once (mp_seq_load); the *_resident scans use it.
        Records may all be empty: the library refuses a null text with n_rows > 0, so a text of no bytes still goes as a valid pointer."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        row_off = np.ascontiguousarray(row_off, dtype=np.int64)
        if not len(data):
            data = np.zeros(1, np.uint8)
        self._ck(self.d.mp_seq_load(self.h, _ptr(data), _ptr(row_off), len(row_off) - 1))

    def seq_free(self):
        self._ck(self.d.mp_seq_free(self.h))

    def seq_info(self):
        """(sequences, bases, bytes on the device) of the store."""
        n, b, d = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self._ck(self.d.mp_seq_info(self.h, C.byref(n), C.byref(b), C.byref(d)))
        return n.value, b.value, d.value

    def pcr_scan_resident(self, codes, off) -> np.ndarray:
        """pcr_scan on the stored database."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int32)
        n_rows, n_pairs = self.seq_info()[0], (len(off) - 1) // 2
        out = np.full((max(n_pairs, 1), max(n_rows, 1), 4), -1, np.int32)
        self._ck(self.d.mp_pcr_scan_resident(self.h, n_pairs, _ptr(codes), _ptr(off), _ptr(out)))
        return out[:n_pairs, :n_rows]

    def kmm_scan_resident(self, pat_codes, pat_off, max_mismatch: int, term: int, cap: int = 1 << 20) -> np.ndarray:
        """kmm_scan on the stored database."""
        pat_codes = np.ascontiguousarray(pat_codes, dtype=np.uint8)
        pat_off = np.ascontiguousarray(pat_off, dtype=np.int32)
        while True:
            hits = np.empty((max(cap, 1), 4), np.int32)
            n = C.c_int64(0)
            self._ck(self.d.mp_kmm_scan_resident(self.h, len(pat_off) - 1, _ptr(pat_codes), _ptr(pat_off), int(max_mismatch), int(term), cap,
                                                 _ptr(hits), C.byref(n)))
            if n.value <= cap:
                h = hits[: n.value]
                return h[np.lexsort((h[:, 3], h[:, 2], h[:, 1], h[:, 0]))] if len(h) else h
            cap = int(n.value)

    def kmm_gap_scan_resident(self, pat_codes, pat_off, max_penalty: int, max_gap: int, term: int, cap: int = 1 << 20) -> np.ndarray:
        """kmm_scan_resident under the gapped rule of include/mprime_offtarget.h: one gap of up to `max_gap` bases beside the mismatches,
        6 per mismatch and 5 + 3 g per gap within `max_penalty`."""
        if not self.lib.gapscan:
            raise MprimeError(-2, f"{self.lib.path} has no gapped scan (libmprime_hip.so does; validate.gap_scan_host is its host form)")
        pat_codes = np.ascontiguousarray(pat_codes, dtype=np.uint8)
        pat_off = np.ascontiguousarray(pat_off, dtype=np.int32)
        while True:
            hits = np.empty((max(cap, 1), 4), np.int32)
            n = C.c_int64(0)
            self._ck(self.d.mp_kmm_gap_scan_resident(self.h, len(pat_off) - 1, _ptr(pat_codes), _ptr(pat_off), int(max_penalty), int(max_gap),
                                                     int(term), cap, _ptr(hits), C.byref(n)))
            if n.value <= cap:
                h = hits[: n.value]
                return h[np.lexsort((h[:, 3], h[:, 2], h[:, 1], h[:, 0]))] if len(h) else h
            cap = int(n.value)

    # include/mprime_offtarget.h
    def _need_offtarget(self):
        if not self.lib.offtarget:
            raise MprimeError(-2, f"{self.lib.path} does not serve include/mprime_offtarget.h (libmprime_hip.so does)")

    def offtarget_resident(self, pat_codes, pat_off, read_primer, max_mismatch, term: int, size_lo: int, size_hi: int, cap: int = 1 << 20) -> np.ndarray:
        """Products [n][6] = (sequence, start, stop, forward primer id, reverse primer id, length) of the off-target screen of the stored
        database, in the order of the report.  Patterns are the reads in ascending read order; max_mismatch per read (or one for all).
        A result larger than `cap` is fetched again with the exact size: the library kept it, nothing is scanned twice."""
        self._need_offtarget()
        pat_codes = np.ascontiguousarray(pat_codes, dtype=np.uint8)
        pat_off = np.ascontiguousarray(pat_off, dtype=np.int32)
        n_pat = len(pat_off) - 1
        read_primer = np.ascontiguousarray(read_primer, dtype=np.int32)
        mm = np.ascontiguousarray(np.broadcast_to(np.asarray(max_mismatch, np.int32), (n_pat,)), dtype=np.int32)
        while True:
            out = np.empty((max(cap, 1), 6), np.int32)
            n = C.c_int64(0)
            self._ck(self.d.mp_offtarget_resident(self.h, n_pat, _ptr(pat_codes), _ptr(pat_off), _ptr(read_primer), _ptr(mm), int(term),
                                                  int(size_lo), int(size_hi), cap, _ptr(out), C.byref(n)))
            if n.value <= cap:
                return out[: n.value]
            cap = int(n.value)

    def offtarget_gap_resident(self, pat_codes, pat_off, read_primer, max_penalty, max_gap: int, term: int, size_lo: int, size_hi: int,
                               cap: int = 1 << 20) -> np.ndarray:
        """offtarget_resident under the gapped rule: max_penalty per read (or one for all), one gap of up to `max_gap` bases."""
        self._need_offtarget()
        pat_codes = np.ascontiguousarray(pat_codes, dtype=np.uint8)
        pat_off = np.ascontiguousarray(pat_off, dtype=np.int32)
        n_pat = len(pat_off) - 1
        read_primer = np.ascontiguousarray(read_primer, dtype=np.int32)
        pen = np.ascontiguousarray(np.broadcast_to(np.asarray(max_penalty, np.int32), (n_pat,)), dtype=np.int32)
        while True:
            out = np.empty((max(cap, 1), 6), np.int32)
            n = C.c_int64(0)
            self._ck(self.d.mp_offtarget_gap_resident(self.h, n_pat, _ptr(pat_codes), _ptr(pat_off), _ptr(read_primer), _ptr(pen), int(max_gap),
                                                      int(term), int(size_lo), int(size_hi), cap, _ptr(out), C.byref(n)))
            if n.value <= cap:
                return out[: n.value]
            cap = int(n.value)

    def amplicon_join(self, sites, size_lo: int, size_hi: int, cap: int = 1 << 20) -> np.ndarray:
        """The join alone: sites [n][4] = (strand, row, position, primer id), strictly ascending in (strand, row, position); products
        [n][6] as offtarget_resident, rows ascending."""
        self._need_offtarget()
        sites = np.ascontiguousarray(sites, dtype=np.int32).reshape(-1, 4)
        while True:
            out = np.empty((max(cap, 1), 6), np.int32)
            n = C.c_int64(0)
            self._ck(self.d.mp_amplicon_join(self.h, len(sites), _ptr(sites), int(size_lo), int(size_hi), cap, _ptr(out), C.byref(n)))
            if n.value <= cap:
                return out[: n.value]
            cap = int(n.value)

    def offtarget_stats(self):
        """Of the last offtarget_resident / amplicon_join: ({scan, reduce, join, call}_ms, {hits, sites and sequences per strand, products})."""
        self._need_offtarget()
        ms, counts = np.zeros(4, np.float64), np.zeros(7, np.int64)
        self._ck(self.d.mp_offtarget_stats(self.h, _ptr(ms), _ptr(counts)))
        return (dict(zip(("scan_ms", "reduce_ms", "join_ms", "call_ms"), ms.tolist())),
                dict(zip(("hits", "forward_sites", "reverse_sites", "products", "forward_genes", "reverse_genes", "both_genes"), counts.tolist())))

    # include/mprime_panel.h
    def _need_panel(self):
        if not self.lib.panel:
            raise MprimeError(-2, f"{self.lib.path} does not serve include/mprime_panel.h (libmprime_hip.so does)")

    def dimer_cross(self, codes, off, jobs, loss_hit, dg_params, dg_limit: float, cap: int = 1 << 16) -> np.ndarray:
        """Hit records [n][6] = (job, y, end length, end expansion, y expansion, idx) of the jobs [m][3] = (x, y_lo, y_hi), sorted by
        (job, y).  A result larger than `cap` is searched again with the exact size."""
        self._need_panel()
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int32)
        jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 3)
        loss_hit = np.ascontiguousarray(loss_hit, dtype=np.uint8)
        dg_params = np.ascontiguousarray(dg_params, dtype=np.float64)
        while True:
            hits = np.empty((max(cap, 1), 6), np.int32)
            n = C.c_int64(0)
            self._ck(self.d.mp_dimer_cross(self.h, len(off) - 1, _ptr(codes), _ptr(off), len(jobs), _ptr(jobs), _ptr(loss_hit),
                                           _ptr(dg_params), dg_limit, cap, _ptr(hits), C.byref(n)))
            if n.value <= cap:
                h = hits[: n.value]
                return h[np.lexsort((h[:, 1], h[:, 0]))] if len(h) else h
            cap = int(n.value)

    def dimer_cross_raw(self, codes, off, jobs, loss_hit, dg_params, dg_limit: float, cap: int):
        """One mp_dimer_cross call as it is: (the first min(cap, n) records in arrival order, n)."""
        self._need_panel()
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int32)
        jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 3)
        loss_hit = np.ascontiguousarray(loss_hit, dtype=np.uint8)
        dg_params = np.ascontiguousarray(dg_params, dtype=np.float64)
        hits = np.empty((max(cap, 1), 6), np.int32)
        n = C.c_int64(0)
        self._ck(self.d.mp_dimer_cross(self.h, len(off) - 1, _ptr(codes), _ptr(off), len(jobs), _ptr(jobs), _ptr(loss_hit),
                                       _ptr(dg_params), dg_limit, cap, _ptr(hits) if cap else None, C.byref(n)))
        return hits[: min(cap, n.value)], int(n.value)

    def amplicon_join_classes(self, sites, size_lo: int, size_hi: int, cap: int = 1 << 20) -> np.ndarray:
        """The three class joins alone: sites [n][5] = (class, strand, row, position, read), strictly ascending in (class, strand, row,
        position); products [n][7] = (row, start, stop, forward read, reverse read, length, join class)."""
        self._need_panel()
        sites = np.ascontiguousarray(sites, dtype=np.int32).reshape(-1, 5)
        while True:
            out = np.empty((max(cap, 1), 7), np.int32)
            n = C.c_int64(0)
            self._ck(self.d.mp_amplicon_join_classes(self.h, len(sites), _ptr(sites), int(size_lo), int(size_hi), cap, _ptr(out), C.byref(n)))
            if n.value <= cap:
                return out[: n.value]
            cap = int(n.value)

    def offtarget_classes(self, pat_codes, pat_off, read_id, read_class, max_mismatch, term: int, size_lo: int, size_hi: int,
                          cap: int = 1 << 20) -> np.ndarray:
        """offtarget_resident with a class (0 core, 1 new) per read: products [n][7] of the three class joins.  A result larger than
        `cap` is fetched again with the exact size: the library kept it, nothing is scanned twice."""
        self._need_panel()
        pat_codes = np.ascontiguousarray(pat_codes, dtype=np.uint8)
        pat_off = np.ascontiguousarray(pat_off, dtype=np.int32)
        n_pat = len(pat_off) - 1
        read_id = np.ascontiguousarray(read_id, dtype=np.int32)
        read_class = np.ascontiguousarray(read_class, dtype=np.int32)
        mm = np.ascontiguousarray(np.broadcast_to(np.asarray(max_mismatch, np.int32), (n_pat,)), dtype=np.int32)
        while True:
            out = np.empty((max(cap, 1), 7), np.int32)
            n = C.c_int64(0)
            self._ck(self.d.mp_offtarget_classes(self.h, n_pat, _ptr(pat_codes), _ptr(pat_off), _ptr(read_id), _ptr(read_class), _ptr(mm),
                                                 int(term), int(size_lo), int(size_hi), cap, _ptr(out), C.byref(n)))
            if n.value <= cap:
                return out[: n.value]
            cap = int(n.value)

    # include/mprime_setscreen.h
    def _need_setscreen(self):
        if not self.lib.setscreen:
            raise MprimeError(-2, f"{self.lib.path} does not serve include/mprime_setscreen.h (libmprime_hip.so does)")

    @staticmethod
    def _sorted_triples(t):
        return t[np.lexsort((t[:, 1], t[:, 0]))] if len(t) else t

    def setscreen_begin(self, size_lo: int, size_hi: int, max_mismatch: int, term: int):
        """Open the set screen of this context on the store of seq_load: products with size_lo < length < size_hi."""
        self._need_setscreen()
        self._ck(self.d.mp_setscreen_begin(self.h, int(size_lo), int(size_hi), int(max_mismatch), int(term)))

    def setscreen_add_raw(self, pat_codes, pat_off, read_primer, cap: int):
        """One mp_setscreen_add call as it is: (the first min(cap, n) triples in arrival order, n)."""
        self._need_setscreen()
        pat_codes = np.ascontiguousarray(pat_codes, dtype=np.uint8)
        pat_off = np.ascontiguousarray(pat_off, dtype=np.int32)
        read_primer = np.ascontiguousarray(read_primer, dtype=np.int32)
        out = np.empty((max(cap, 1), 3), np.int64)
        n = C.c_int64(0)
        self._ck(self.d.mp_setscreen_add(self.h, len(pat_off) - 1, _ptr(pat_codes), _ptr(pat_off), _ptr(read_primer), cap,
                                         _ptr(out) if cap else None, C.byref(n)))
        return out[: min(cap, n.value)], int(n.value)

    def setscreen_add(self, pat_codes, pat_off, read_primer, cap: int = 1 << 16, with_stats: bool = False):
        """Screen the reads of new primers (read_primer: global primer ids, non-decreasing, above every earlier id).  Triples [n][3]
        int64 = (A, B, products(A -> B)) of the ordered pairs with a new primer and a product, sorted by (A, B).  A result larger than
        `cap` is fetched again with the exact size: the library kept it, nothing is scanned twice.  with_stats: (triples,
        setscreen_stats() of the call that scanned — the fetch that follows it reports zeros)."""
        t, n = self.setscreen_add_raw(pat_codes, pat_off, read_primer, cap)
        stats = self.setscreen_stats() if with_stats else None
        if n > cap:
            t, n = self.setscreen_add_raw(pat_codes, pat_off, read_primer, n)
        t = self._sorted_triples(t)
        return (t, stats) if with_stats else t

    def setscreen_site_counts(self, first: int, n: int):
        """(forward, reverse) int64 [n]: the de-duplicated sites of primers first .. first + n - 1."""
        self._need_setscreen()
        f, r = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        self._ck(self.d.mp_setscreen_site_counts(self.h, int(first), int(n), _ptr(f), _ptr(r)))
        return f[:n], r[:n]

    def setscreen_stats(self):
        """Of the last setscreen_add / setscreen_join: ({scan, bin, join, call}_ms, counts)."""
        self._need_setscreen()
        ms, counts = np.zeros(4, np.float64), np.zeros(8, np.int64)
        self._ck(self.d.mp_setscreen_stats(self.h, _ptr(ms), _ptr(counts)))
        return (dict(zip(("scan_ms", "bin_ms", "join_ms", "call_ms"), ms.tolist())),
                dict(zip(("scan_launches", "list_regrows", "table_regrows", "forward_sites", "reverse_sites", "pairs", "products", "adds"),
                         counts.tolist())))

    def setscreen_end(self):
        self._need_setscreen()
        self._ck(self.d.mp_setscreen_end(self.h))

    def setscreen_join(self, sites, size_lo: int, size_hi: int, cap: int = 1 << 16) -> np.ndarray:
        """The join alone: sites [n][4] = (strand, row, position, primer id), strictly ascending; triples as setscreen_add."""
        self._need_setscreen()
        sites = np.ascontiguousarray(sites, dtype=np.int32).reshape(-1, 4)
        while True:
            out = np.empty((max(cap, 1), 3), np.int64)
            n = C.c_int64(0)
            self._ck(self.d.mp_setscreen_join(self.h, len(sites), _ptr(sites), int(size_lo), int(size_hi), cap, _ptr(out), C.byref(n)))
            if n.value <= cap:
                return self._sorted_triples(out[: n.value])
            cap = int(n.value)

    # include/mprime_anchor.h
    def _need_anchor(self):
        if not self.lib.anchor:
            raise MprimeError(-2, f"{self.lib.path} does not serve include/mprime_anchor.h (libmprime_hip.so does)")

    def anchor_set(self, anchor, col, width: int, band: int = 32, match: int = 5, mismatch: int = 4, gap_open: int = 10, gap_extend: int = 2,
                   min_identity_permille: int = 500):
        """Keep the anchor (upper-case letters, bytes or uint8 array) and its seed columns in the context (mp_anchor_set)."""
        self._need_anchor()
        codes = np.ascontiguousarray(np.frombuffer(anchor, np.uint8) if isinstance(anchor, (bytes, bytearray)) else anchor, dtype=np.uint8)
        col = np.ascontiguousarray(col, dtype=np.int32)
        par = AnchorParams(int(match), int(mismatch), int(gap_open), int(gap_extend), int(band), int(min_identity_permille))
        self._ck(self.d.mp_anchor_set(self.h, _ptr(codes), len(codes), _ptr(col), int(width), C.byref(par)))
        self.anchor_n, self.anchor_width = len(codes), int(width)

    def anchor_align(self, data, off, want_ops: bool = False):
        """(rows uint8 [n][width], meta int32 [n][ANCHOR_META], ops): the queries data[off[q]:off[q+1]] placed on the anchor.  ops: a list
        of byte strings over M / D / I when asked for, else None."""
        self._need_anchor()
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        nq = len(off) - 1
        rows = np.empty((max(nq, 1), self.anchor_width), np.uint8)
        meta = np.zeros((max(nq, 1), ANCHOR_META), np.int32)
        ops_off = ops_buf = None
        if want_ops:
            ops_off = np.ascontiguousarray(off + np.arange(nq + 1, dtype=np.int64) * self.anchor_n)       # a slot of m + n bytes per query
            ops_buf = np.zeros(max(int(ops_off[-1]), 1), np.uint8)
        self._ck(self.d.mp_anchor_align(self.h, nq, _ptr(data), _ptr(off), int(want_ops), _ptr(rows), _ptr(meta), _ptr(ops_buf), _ptr(ops_off)))
        ops = None
        if want_ops:                               # right-aligned in its slot, m + n_del letters
            length = np.diff(off) + meta[:nq, 4]
            ops = [ops_buf[int(ops_off[q + 1]) - int(length[q]): int(ops_off[q + 1])].tobytes() if meta[q, 0] != -(1 << 31) else b""
                   for q in range(nq)]
        return rows[:nq], meta[:nq], ops

    def anchor_strands(self, both: bool = True):
        """Switch of the context (mp_anchor_strands): anchor_align and star_round vote both strands and turn a query once; meta status
        bit 3 (ANCHOR_REVERSED) marks a turned one."""
        self._need_anchor()
        if not self.lib.strands:
            raise MprimeError(-2, f"{self.lib.path} has no both-strand entry points")
        self._ck(self.d.mp_anchor_strands(self.h, int(bool(both))))

    def anchor_stats(self):
        """Of the last anchor_align: ({vote, dp, trace, readback, call}_ms, {batches, cells, traceback_bytes})."""
        self._need_anchor()
        ms, counts = np.zeros(5, np.float64), np.zeros(3, np.int64)
        self._ck(self.d.mp_anchor_stats(self.h, _ptr(ms), _ptr(counts)))
        return (dict(zip(("vote_ms", "dp_ms", "trace_ms", "readback_ms", "call_ms"), ms.tolist())),
                dict(zip(("batches", "cells", "traceback_bytes"), counts.tolist())))

    # include/mprime_cluster.h
    def _need_cluster(self):
        if not self.lib.cluster:
            raise MprimeError(-2, f"{self.lib.path} does not serve include/mprime_cluster.h (libmprime_hip.so does)")

    def cluster_load(self, data, off):
        """Make the sequences data[off[i]:off[i+1]] resident (mp_cluster_load)."""
        self._need_cluster()
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        self._ck(self.d.mp_cluster_load(self.h, len(off) - 1, _ptr(data), _ptr(off)))
        self.cluster_n = len(off) - 1

    @staticmethod
    def _cluster_params(band, identity_permille, min_votes, match, mismatch, gap_open, gap_extend):
        return ClusterParams(int(match), int(mismatch), int(gap_open), int(gap_extend), int(band), int(identity_permille), int(min_votes))

    def cluster_pairs(self, q_idx, r_idx, band: int = 32, identity_permille: int = 800, min_votes: int = 1, match: int = 5, mismatch: int = 4,
                      gap_open: int = 10, gap_extend: int = 2) -> np.ndarray:
        """int32 [n_pairs][CLUSTER_PAIR] = votes, d0, score, n_match, status of query q_idx[p] against anchor r_idx[p] (mp_cluster_pairs)."""
        self._need_cluster()
        q_idx = np.ascontiguousarray(q_idx, dtype=np.int32)
        r_idx = np.ascontiguousarray(r_idx, dtype=np.int32)
        out = np.zeros((max(len(q_idx), 1), CLUSTER_PAIR), np.int32)
        par = self._cluster_params(band, identity_permille, min_votes, match, mismatch, gap_open, gap_extend)
        self._ck(self.d.mp_cluster_pairs(self.h, len(q_idx), _ptr(q_idx), _ptr(r_idx), C.byref(par), _ptr(out)))
        return out[: len(q_idx)]

    def cluster_greedy(self, band: int = 32, identity_permille: int = 800, min_votes: int = 1, match: int = 5, mismatch: int = 4,
                       gap_open: int = 10, gap_extend: int = 2):
        """(cluster_of int32 [n], rep_of_cluster int32 [n_clusters], n_match_of int32 [n]) of the resident sequences (mp_cluster_greedy)."""
        self._need_cluster()
        n = getattr(self, "cluster_n", 0)
        cluster_of, rep, n_match = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        nc = C.c_int32(0)
        par = self._cluster_params(band, identity_permille, min_votes, match, mismatch, gap_open, gap_extend)
        self._ck(self.d.mp_cluster_greedy(self.h, C.byref(par), _ptr(cluster_of), _ptr(rep), _ptr(n_match), C.byref(nc)))
        return cluster_of[:n], rep[: nc.value], n_match[:n]

    def cluster_pairs_strands(self, q_idx, r_idx, q_strand, band: int = 32, identity_permille: int = 800, min_votes: int = 1, match: int = 5,
                              mismatch: int = 4, gap_open: int = 10, gap_extend: int = 2):
        """cluster_pairs with a strand per pair: q_strand[p] = 1 takes the reverse complement of q_idx[p] as the query (mp_cluster_pairs_strands)."""
        self._need_cluster()
        if not self.lib.strands:
            raise MprimeError(-2, f"{self.lib.path} has no both-strand entry points")
        q_idx, r_idx = np.ascontiguousarray(q_idx, dtype=np.int32), np.ascontiguousarray(r_idx, dtype=np.int32)
        q_strand = np.ascontiguousarray(q_strand, dtype=np.int32)
        if not len(q_idx) == len(r_idx) == len(q_strand):
            raise ValueError("cluster_pairs_strands: q_idx, r_idx and q_strand differ in length")
        out = np.zeros((max(len(q_idx), 1), CLUSTER_PAIR), np.int32)
        par = self._cluster_params(band, identity_permille, min_votes, match, mismatch, gap_open, gap_extend)
        self._ck(self.d.mp_cluster_pairs_strands(self.h, len(q_idx), _ptr(q_idx), _ptr(r_idx), _ptr(q_strand), C.byref(par), _ptr(out)))
        return out[: len(q_idx)]

    def cluster_greedy_strands(self, band: int = 32, identity_permille: int = 800, min_votes: int = 1, match: int = 5, mismatch: int = 4,
                               gap_open: int = 10, gap_extend: int = 2):
        """(cluster_of, rep_of_cluster, n_match_of, strand_of int32 [n]) under both strands (mp_cluster_greedy_strands)."""
        self._need_cluster()
        if not self.lib.strands:
            raise MprimeError(-2, f"{self.lib.path} has no both-strand entry points")
        n = getattr(self, "cluster_n", 0)
        cluster_of, rep, n_match, strand = (np.zeros(max(n, 1), np.int32) for _ in range(4))
        nc = C.c_int32(0)
        par = self._cluster_params(band, identity_permille, min_votes, match, mismatch, gap_open, gap_extend)
        self._ck(self.d.mp_cluster_greedy_strands(self.h, C.byref(par), _ptr(cluster_of), _ptr(rep), _ptr(n_match), _ptr(strand), C.byref(nc)))
        return cluster_of[:n], rep[: nc.value], n_match[:n], strand[:n]

    def cluster_stats(self):
        """Of the last cluster_greedy / cluster_pairs: ({index, seed, dp, resolve, call}_ms, {rounds, pairs, cells})."""
        self._need_cluster()
        ms, counts = np.zeros(5, np.float64), np.zeros(3, np.int64)
        self._ck(self.d.mp_cluster_stats(self.h, _ptr(ms), _ptr(counts)))
        return (dict(zip(("index_ms", "seed_ms", "dp_ms", "resolve_ms", "call_ms"), ms.tolist())),
                dict(zip(("rounds", "pairs", "cells"), counts.tolist())))

    # include/mprime_star.h
    def _need_star(self):
        if not self.lib.star:
            raise MprimeError(-2, f"{self.lib.path} does not serve include/mprime_star.h (libmprime_hip.so does)")

    def star_load(self, data, off):
        """Make the records data[off[q]:off[q+1]] resident (mp_star_load)."""
        self._need_star()
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        self.star_n = 0
        self._ck(self.d.mp_star_load(self.h, len(off) - 1, _ptr(data), _ptr(off)))
        self.star_n = len(off) - 1

    def star_round(self, anchor, band: int = 32, match: int = 5, mismatch: int = 4, gap_open: int = 10, gap_extend: int = 2,
                   min_identity_permille: int = 500):
        """One round against `anchor` (mp_star_round): (meta int32 [n_records][STAR_META], ins int32 [n + 1], width)."""
        self._need_star()
        codes = np.ascontiguousarray(np.frombuffer(anchor, np.uint8) if isinstance(anchor, (bytes, bytearray)) else anchor, dtype=np.uint8)
        n_rec = getattr(self, "star_n", 0)
        meta = np.zeros((max(n_rec, 1), STAR_META), np.int32)
        ins = np.zeros(len(codes) + 1, np.int32)
        width = C.c_int32(0)
        par = AnchorParams(int(match), int(mismatch), int(gap_open), int(gap_extend), int(band), int(min_identity_permille))
        self.star_width = 0
        self._ck(self.d.mp_star_round(self.h, _ptr(codes), len(codes), C.byref(par), _ptr(meta), _ptr(ins), C.byref(width)))
        self.star_width = int(width.value)
        return meta[:n_rec], ins, self.star_width

    def star_rows(self) -> np.ndarray:
        """uint8 [n_records][width]: the rows of the last round, all-gap for the unplaced records (mp_star_rows)."""
        self._need_star()
        rows = np.empty((max(getattr(self, "star_n", 0), 1), max(getattr(self, "star_width", 0), 1)), np.uint8)
        self._ck(self.d.mp_star_rows(self.h, _ptr(rows)))
        return rows[: self.star_n]

    def star_counts(self) -> np.ndarray:
        """int32 [width][STAR_COUNTS]: A, C, G, T, other letter, gap per column over the placed rows of the last round (mp_star_counts)."""
        self._need_star()
        counts = np.zeros((max(getattr(self, "star_width", 0), 1), STAR_COUNTS), np.int32)
        self._ck(self.d.mp_star_counts(self.h, _ptr(counts)))
        return counts[: self.star_width]

    def star_stats(self):
        """Of the last star_round: ({vote, dp, trace, profile, write, count, readback, call}_ms, {batches, cells, realigned,
        traceback_bytes, store_bytes, placed})."""
        self._need_star()
        ms, counts = np.zeros(8, np.float64), np.zeros(6, np.int64)
        self._ck(self.d.mp_star_stats(self.h, _ptr(ms), _ptr(counts)))
        return (dict(zip(("vote_ms", "dp_ms", "trace_ms", "profile_ms", "write_ms", "count_ms", "readback_ms", "call_ms"), ms.tolist())),
                dict(zip(("batches", "cells", "realigned", "traceback_bytes", "store_bytes", "placed"), counts.tolist())))

    def star_free(self):
        self._need_star()
        self._ck(self.d.mp_star_free(self.h))
        self.star_n = self.star_width = 0

    # include/mprime_ani.h
    def _need_ani(self):
        if not self.lib.ani:
            raise MprimeError(-2, f"{self.lib.path} does not serve include/mprime_ani.h (libmprime_hip.so does)")

    def _need_ani_strands(self):
        self._need_ani()
        if not self.lib.ani_strands:
            raise MprimeError(-2, f"{self.lib.path} has no both-strand entry points of include/mprime_ani.h")

    def ani_sketch(self, data, off, s: int = ANI_MAX_SKETCH, strands: bool = False):
        """Sketch the sequences data[off[i]:off[i+1]] at size s and keep the sketches resident (mp_ani_sketch); strands: canonical
        sketches with their orientation bits (mp_ani_sketch_strands)."""
        self._need_ani_strands() if strands else self._need_ani()
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        rc = (self.d.mp_ani_sketch_strands if strands else self.d.mp_ani_sketch)(self.h, len(off) - 1, _ptr(data), _ptr(off), int(s))
        if rc != 0 and rc != -1:                # (MP_ERR_ARG: refused before anything was touched, the earlier set stays resident)
            self.ani_n = 0
        self._ck(rc)
        self.ani_n, self.ani_s = len(off) - 1, int(s)

    def ani_sketches(self):
        """(hashes uint32 [n][s], sizes int32 [n]) of the resident sketches; a sketch is hashes[i, :sizes[i]] (mp_ani_sketches)."""
        self._need_ani()
        n, s = getattr(self, "ani_n", 0), getattr(self, "ani_s", 0)
        hashes, sizes = np.zeros((max(n, 1), max(s, 1)), np.uint32), np.zeros(max(n, 1), np.int32)
        self._ck(self.d.mp_ani_sketches(self.h, _ptr(hashes), _ptr(sizes)))
        return hashes[:n], sizes[:n]

    def ani_pairs(self, a_idx, b_idx) -> np.ndarray:
        """int32 [n_pairs][ANI_PAIR] = w, u, ani_ppm of sketch a_idx[p] against sketch b_idx[p] (mp_ani_pairs)."""
        self._need_ani()
        a_idx = np.ascontiguousarray(a_idx, dtype=np.int32)
        b_idx = np.ascontiguousarray(b_idx, dtype=np.int32)
        out = np.zeros((max(len(a_idx), 1), ANI_PAIR), np.int32)
        self._ck(self.d.mp_ani_pairs(self.h, len(a_idx), _ptr(a_idx), _ptr(b_idx), _ptr(out)))
        return out[: len(a_idx)]

    def ani_groups(self, group_off, q_group, r_group, report_ppm: int = 700000) -> np.ndarray:
        """int64 [n_gp][2] = n_rep, sum_ppm of group q_group[x] against group r_group[x]; group g is the resident sequences
        group_off[g] .. group_off[g+1] (mp_ani_groups)."""
        self._need_ani()
        group_off = np.ascontiguousarray(group_off, dtype=np.int32)
        q_group = np.ascontiguousarray(q_group, dtype=np.int32)
        r_group = np.ascontiguousarray(r_group, dtype=np.int32)
        out = np.zeros((max(len(q_group), 1), 2), np.int64)
        self._ck(self.d.mp_ani_groups(self.h, len(group_off) - 1, _ptr(group_off), len(q_group), _ptr(q_group), _ptr(r_group), int(report_ppm),
                                      _ptr(out)))
        return out[: len(q_group)]

    def ani_orientations(self) -> np.ndarray:
        """uint32 [n][(s + 31) // 32]: the orientation bits of the resident canonical sketches, bit i % 32 of word i // 32 for entry i
        (mp_ani_orientations)."""
        self._need_ani_strands()
        n, s = getattr(self, "ani_n", 0), getattr(self, "ani_s", 0)
        bits = np.zeros((max(n, 1), max((s + 31) // 32, 1)), np.uint32)
        self._ck(self.d.mp_ani_orientations(self.h, _ptr(bits)))
        return bits[:n]

    def ani_pairs_strand(self, a_idx, b_idx) -> np.ndarray:
        """int32 [n_pairs][2] = same, opp of canonical sketch a_idx[p] against canonical sketch b_idx[p] (mp_ani_pairs_strand)."""
        self._need_ani_strands()
        a_idx = np.ascontiguousarray(a_idx, dtype=np.int32)
        b_idx = np.ascontiguousarray(b_idx, dtype=np.int32)
        out = np.zeros((max(len(a_idx), 1), 2), np.int32)
        self._ck(self.d.mp_ani_pairs_strand(self.h, len(a_idx), _ptr(a_idx), _ptr(b_idx), _ptr(out)))
        return out[: len(a_idx)]

    def ani_groups_strand(self, group_off, q_group, r_group, report_ppm: int = 700000) -> np.ndarray:
        """int64 [n_gp][2] = SAME, OPP of group q_group[x] against group r_group[x] over the pairs reported at the floor
        (mp_ani_groups_strand); groups as in ani_groups."""
        self._need_ani_strands()
        group_off = np.ascontiguousarray(group_off, dtype=np.int32)
        q_group = np.ascontiguousarray(q_group, dtype=np.int32)
        r_group = np.ascontiguousarray(r_group, dtype=np.int32)
        out = np.zeros((max(len(q_group), 1), 2), np.int64)
        self._ck(self.d.mp_ani_groups_strand(self.h, len(group_off) - 1, _ptr(group_off), len(q_group), _ptr(q_group), _ptr(r_group),
                                             int(report_ppm), _ptr(out)))
        return out[: len(q_group)]

    def ani_table(self) -> np.ndarray:
        return self.lib.ani_table()

    def ani_stats(self):
        """({sketch, compare}_ms, {sketches, pairs}): device event times of the last ani_sketch and of the comparisons since."""
        self._need_ani()
        ms, counts = np.zeros(2, np.float64), np.zeros(2, np.int64)
        self._ck(self.d.mp_ani_stats(self.h, _ptr(ms), _ptr(counts)))
        return dict(zip(("sketch_ms", "compare_ms"), ms.tolist())), dict(zip(("sketches", "pairs"), counts.tolist()))

    # include/mprime_dege.h
    def _need_dege(self):
        if not self.lib.dege:
            raise MprimeError(-2, f"{self.lib.path} does not serve include/mprime_dege.h (libmprime_hip.so does)")

    def dege_load(self, rows):
        """Upload a trimmed alignment: rows uint8 [n_rows][width] (mp_dege_load)."""
        self._need_dege()
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        if rows.ndim != 2:
            raise ValueError("dege_load: rows must be a matrix of bytes")
        self.dege_n_win = self.dege_iters = 0
        self._ck(self.d.mp_dege_load(self.h, rows.shape[0], rows.shape[1], _ptr(rows)))

    def dege_windows(self, l: int, skip: int = 20, depth: int = 1):
        """(nums int32 [W][DEGE_WIN] = NumberSpanning, Z, UniqueMers, printed; entropy float64 [W]) of every window (mp_dege_windows,
        mp_dege_window_table)."""
        self._need_dege()
        n = C.c_int32(0)
        self.dege_n_win = self.dege_iters = 0
        self._ck(self.d.mp_dege_windows(self.h, int(l), int(skip), int(depth), C.byref(n)))
        self.dege_n_win = n.value
        nums, ent = np.zeros((n.value, DEGE_WIN), np.int32), np.zeros(n.value, np.float64)
        self._ck(self.d.mp_dege_window_table(self.h, _ptr(nums), _ptr(ent)))
        self.dege_nums = nums
        return nums, ent

    def dege_unique(self, pos: int):
        """(words uint64 [U] ascending, counts int32 [U]) of window pos (mp_dege_unique)."""
        self._need_dege()
        if not 0 <= pos < getattr(self, "dege_n_win", 0):
            raise MprimeError(-1, f"dege_unique: window {pos} of {getattr(self, 'dege_n_win', 0)}")
        u = int(self.dege_nums[pos, 2])
        words, counts = np.zeros(u, np.uint64), np.zeros(u, np.int32)
        self._ck(self.d.mp_dege_unique(self.h, int(pos), u, _ptr(words), _ptr(counts)))
        return words, counts

    def dege_merge(self, max_deg: int, iters: int = 100, seed: int = 0) -> np.ndarray:
        """int32 [W][DEGE_REC] = match, deg, iteration, sets[32] of every window's winning iteration, -1 where the window is not printed
        (mp_dege_merge, mp_dege_best)."""
        self._need_dege()
        if not 1 <= int(max_deg) <= 0x7FFFFFFF:
            raise MprimeError(-1, f"dege_merge: maximum degeneracy {max_deg} (1..2147483647)")
        self._ck(self.d.mp_dege_merge(self.h, int(max_deg), int(iters), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)))
        self.dege_iters = int(iters)
        out = np.zeros((self.dege_n_win, DEGE_REC), np.int32)
        self._ck(self.d.mp_dege_best(self.h, _ptr(out)))
        return out

    def dege_iterations(self, pos: int) -> np.ndarray:
        """int32 [iters][DEGE_REC] = deg, match, n_draws, sets[32] of every iteration of one printed window (mp_dege_iterations)."""
        self._need_dege()
        out = np.zeros((getattr(self, "dege_iters", 0), DEGE_REC), np.int32)
        self._ck(self.d.mp_dege_iterations(self.h, int(pos), _ptr(out)))
        return out

    def dege_stats(self):
        """({window, merge}_ms, {windows, printed, unique, global_windows}): device event times and counts of the last calls."""
        self._need_dege()
        ms, counts = np.zeros(2, np.float64), np.zeros(4, np.int64)
        self._ck(self.d.mp_dege_stats(self.h, _ptr(ms), _ptr(counts)))
        return dict(zip(("window_ms", "merge_ms"), ms.tolist())), dict(zip(("windows", "printed", "unique", "global_windows"), counts.tolist()))

    # include/mprime_ont.h
    def _need_ont(self):
        if not self.lib.ont:
            raise MprimeError(-2, f"{self.lib.path} does not serve include/mprime_ont.h (libmprime_hip.so does)")

    def ont_set_keys(self, data, off):
        """Make the keys data[off[i]:off[i+1]] (upper-case A, C, G, T, at most ONT_MAX_LEN bytes each) resident (mp_ont_set_keys)."""
        self._need_ont()
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        if data.size == 0:
            data = np.zeros(1, np.uint8)
        self._ck(self.d.mp_ont_set_keys(self.h, len(off) - 1, _ptr(data), _ptr(off)))

    def ont_assign(self, data, off, q):
        """(key int32 [n], m int32 [n]): per piece data[off[p]:off[p+1]] the resident key of the highest rank q[T][M], the first among
        equals, and its match count (mp_ont_assign).  q: int32 [ONT_Q_ROWS][ONT_Q_COLS]."""
        self._need_ont()
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        q = np.ascontiguousarray(q, dtype=np.int32)
        if q.shape != (ONT_Q_ROWS, ONT_Q_COLS):
            raise ValueError(f"ont_assign: q must be {ONT_Q_ROWS} x {ONT_Q_COLS}")
        if data.size == 0:
            data = np.zeros(1, np.uint8)
        n = len(off) - 1
        key, m = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        self._ck(self.d.mp_ont_assign(self.h, n, _ptr(data), _ptr(off), _ptr(q), _ptr(key), _ptr(m)))
        return key[:n], m[:n]

    def ont_stats(self):
        """({assign_ms}, {keys, pieces}): device event time of the assignment kernels and the counts since the last ont_set_keys."""
        self._need_ont()
        ms, counts = np.zeros(1, np.float64), np.zeros(2, np.int64)
        self._ck(self.d.mp_ont_stats(self.h, _ptr(ms), _ptr(counts)))
        return {"assign_ms": float(ms[0])}, dict(zip(("keys", "pieces"), counts.tolist()))

    def device_bytes(self) -> int:
        b = C.c_int64(0)
        self._ck(self.d.mp_device_bytes(self.h, C.byref(b)))
        return b.value
