/*
 * mprime_subset.h — C ABI of the global-optimum degenerate positions of the core step: `-m multiPrime2` of the reference's
 * test_data/global_optimum/multiPrime2-core_V2.py ("V2": get_Y_position / remove_elements, V2:1236-1291).  Exported by
 * multiprime_amd/csrc/libmprime_hip.so only (csrc/subset.hip); the checker is the plain-Python model tests/subset_ref.py.
 *
 * One SEARCH = one seed (k base indices 0..3 = A, C, G, T) of one window against that window's table of k-mers.
 *   records   every table entry u with at most v gaps other than the seed gives Y(u) = { (i, b) : u[i] != seed[i] }, b = u[i], and for a gap
 *             b = seed[i] (the element counts as a mismatch and changes nothing when merged).  Element id = 4 i + b, so a set of elements
 *             is a 128-bit mask (two uint64, low word first) and k <= MP_SUBSET_MAX_K.
 *   steps     dn = 2 .. N (step index dn - 2; N - 1 steps, none when N < 2).  The records with 1 < |Y| < dn + v are admitted, T = the union
 *             of their elements.  When |T| >= dn every combination S of dn - 1 elements of T gets
 *                 total(S) = sum of the counts of the admitted records with |Y - S| <= v.
 *             Combinations are ranked in lexicographic order of the ascending element ids (itertools.combinations of the sorted list).
 *   results   per (search, step): T, the number of admitted entries, the best total with the LOWEST rank attaining it, the lowest rank
 *             whose total equals the search's cover_number (-1: none), and — only when there is such a rank — the best total over the
 *             ranks below it (what the reference's running maximum holds when its early exit fires).  A step with |T| < dn is not
 *             searched: its totals are 0 and its ranks -1.
 * Two departures from V2, both documented in INTEGRATION.md: the combination order is fixed (V2 draws from a Python set, so its winner
 * among equal totals depends on the hash seed), and the early exit tests a combination's total, not the running sum inside the record loop
 * (the two differ only when a total can exceed cover_number).
 *
 * Refused with MP_ERR_ARG and a message: k > MP_SUBSET_MAX_K; a step whose combination count does not fit 32 bits; a window whose
 * summed counts do not fit 32 bits (the reduction packs a total and a rank into one 64-bit word).
 */
#ifndef MPRIME_SUBSET_H
#define MPRIME_SUBSET_H

#include <stdint.h>

#include "mprime.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MP_SUBSET_MAX_K 32

/* Explicit form.  Window w's entries are [win_off[w], win_off[w+1]) of n = win_off[n_windows] entries; words = b0 at [0,n), b1 at [n,2n),
 * g at [2n,3n) (window words of mprime.h: uint32 while k <= 31, uint64 at k = 32); counts [n] int64.  Search s: window s_window[s], seed
 * s_seed[s*k .. s*k+k), cover_number s_cover[s].  Outputs, indexed [s * (N - 1) + dn - 2] (N < 2: nothing is written):
 *   t_mask [..][2] uint64, n_admitted int32, best_total int64, best_rank int64, exit_rank int64, pre_total int64.
 * An entry listed twice counts twice. */
int mp_subset_search(mp_ctx *ctx, int32_t k, int32_t v, int32_t N, int32_t n_windows, const int64_t *win_off, const void *words,
                     const int64_t *counts, int32_t n_search, const int32_t *s_window, const uint8_t *s_seed, const int64_t *s_cover,
                     uint64_t *t_mask, int32_t *n_admitted, int64_t *best_total, int64_t *best_rank, int64_t *exit_rank,
                     int64_t *pre_total);

/* Resident form: the same over the histogram tables mp_window_unique left in the context (k and v are those of mp_build_windows), plus
 * n_extra extra entries of count 1 each — the expansions of the IUPAC exception rows, which the host owns: x_window[i] (any order),
 * x_words[3*i .. 3*i+2] = b0, b1, g (what mp_expand_exception_words returns).  Same kernels, same outputs. */
int mp_subset_search_resident(mp_ctx *ctx, int32_t N, int64_t n_extra, const int32_t *x_window, const void *x_words, int32_t n_search,
                              const int32_t *s_window, const uint8_t *s_seed, const int64_t *s_cover, uint64_t *t_mask,
                              int32_t *n_admitted, int64_t *best_total, int64_t *best_rank, int64_t *exit_rank, int64_t *pre_total);

/* Device milliseconds of the three kernels of the last search of this context (records, step sets, search incl. the prefix passes). */
int mp_subset_timing(mp_ctx *ctx, double *ms3);

/* Host replay of remove_elements (V2:1261-1291) on the per-step results above — no device, no context:
 *   max_count = 0, subset = {}; for dn = 2 .. N:
 *     |T| >= dn: exit_rank >= 0 ends the search with (max(max_count, pre_total), the combination of that rank);
 *                else best_total > max_count replaces (max_count, subset) by (best_total, the combination of best_rank);
 *     |T| <  dn: max_count = cover_number, subset = T; the loop goes on.
 * Outputs per search: subset [2] uint64 (element mask), max_count, codes [k] = the seed with every element (i, b) of the subset merged
 * into the base set at position i (symbol codes of mprime.h).  Returns MP_ERR_ARG on k > MP_SUBSET_MAX_K or an impossible rank. */
int mp_subset_replay(int32_t k, int32_t N, int32_t n_search, const uint8_t *s_seed, const int64_t *s_cover, const uint64_t *t_mask,
                     const int64_t *best_total, const int64_t *best_rank, const int64_t *exit_rank, const int64_t *pre_total,
                     uint64_t *subset, int64_t *max_count, uint8_t *codes);

/* NM or MM per window (V2:1195-1207): pair p has the NM search nm[p] and the MM search mm[p] (-1: one seed only); NM wins when its
 * max_count >= MM's.  chosen[p] = the search index taken. */
int mp_subset_choose(int32_t n_pairs, const int32_t *nm, const int32_t *mm, const int64_t *max_count, int32_t *chosen);

#ifdef __cplusplus
}
#endif
#endif /* MPRIME_SUBSET_H */
