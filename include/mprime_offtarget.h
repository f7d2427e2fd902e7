/*
 * mprime_offtarget.h — C ABI of the off-target screen (scripts/primer_specificity.py): the k-mismatch scan of the
 * resident sequence store (mprime.h section 8b) with the hits reduced to primer sites and joined into PCR products ON THE DEVICE,
 * so that the host receives products, never hits.  multiprime_amd/csrc/offtarget.hip; exported by libmprime_hip.so only (the
 * oracle library serves mprime.h; the checker of these calls is the host path of multiprime_amd/validate.py: its scan sites through
 * validate.amplicons() and the report code, tests/test_offtarget_gpu.py).
 *
 * Conventions as in mprime.h: MP_OK (0) or a negative MP_ERR_* code, the message in mp_last_error(ctx); the caller owns every buffer.
 *
 * A product is six int32: {row, start, stop, forward primer id, reverse primer id, length}, `start` the 0-based position of a
 * forward site, `stop` that of a reverse-strand site of the same sequence (both as a mapper reports them: the leftmost base of the
 * alignment), length = stop - start + 1.  Per sequence, products follow validate.amplicons() (V9:318-345) exactly: starts ascending,
 * stops ascending, size_lo < length < size_hi; no product at all when stops[0] - starts[-1] > size_hi or stops[-1] - starts[0] <
 * size_lo; and the first start without a stop in [start + size_lo, start + size_hi) ends the sequence's search (later starts give
 * nothing even where they would have a partner).  cap / *n_out as in mp_dimer_scan: *n_out is the number
 * of products, out receives the first min(cap, *n_out) of them.
 */
#ifndef MPRIME_OFFTARGET_H
#define MPRIME_OFFTARGET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct mp_ctx;

/* The whole screen on the store of mp_seq_load.  Patterns: the reads (expanded 3' terms), concrete A/C/G/T, 4..MP_PATTERN_MAX_LEN
 * bases, IN ASCENDING READ ORDER; max_mismatch[i] is read i's budget (mp_kmm_scan's rule with max_mismatch[i] and `term`; reads of
 * different budgets are scanned by one launch per budget), read_primer[i] the id of its primer.
 *   sites      per (strand, sequence, position) the read of the LARGEST index that hits there, reported as its primer id (the host
 *              path sorts hits by read and writes them into a dict: the last write wins);
 *   sequences  in ascending (smallest index of a read with a forward hit on it, sequence) — the order in which the host path's dicts
 *              first see them; only sequences with sites on both strands can give products.
 * The products of the last call stay on the device: a call with the same arguments on the same store that finds *n_out > cap
 * the first time copies them out the second time without scanning again (the store is reloaded or freed: they are dropped). */
int mp_offtarget_resident(struct mp_ctx *ctx, int32_t n_patterns, const uint8_t *pat_codes, const int32_t *pat_off,
                          const int32_t *read_primer, const int32_t *max_mismatch, int32_t term, int32_t size_lo, int32_t size_hi,
                          int64_t cap, int32_t *out, int64_t *n_out);

/* The join alone on explicit sites: sites[4i..] = {strand (0 forward, 1 reverse), row >= 0, position >= 0, primer id}, strictly
 * ascending in (strand, row, position) — one primer per site, as the reduction leaves it.  Rows come out in ascending order.  Runs
 * from scratch on every call (it holds no state). */
int mp_amplicon_join(struct mp_ctx *ctx, int64_t n_sites, const int32_t *sites, int32_t size_lo, int32_t size_hi, int64_t cap,
                     int32_t *out, int64_t *n_out);

/* ---- the gapped rule: bowtie2's end-to-end scoring with at most one short gap ------------------------------------------------------
 * A read of L bases as the text reads it (the read, or its reverse complement on strand 1) hits row T at the 0-based start p when the
 * ungapped rule of mp_kmm_scan holds with max_penalty / 6 mismatches, or when one of these alignments exists for a gap of
 * g = 1 .. max_gap bases and a split c:
 *   type D (c M, g D, (L - c) M)          read base j pairs with T[p + j] for j < c and with T[p + g + j] for j >= c;
 *                                         MP_KMM_GBAR <= c <= L - MP_KMM_GBAR, p + L + g <= len(T); the skipped text bases may be anything
 *   type I (c M, g I, (L - c - g) M)      read base j pairs with T[p + j] for j < c and with T[p + j - g] for j >= c + g;
 *                                         MP_KMM_GBAR <= c, c + g <= L - MP_KMM_GBAR, p + L - g <= len(T)
 * with 6 * mismatches + 5 + 3 * g <= max_penalty (a pair mismatches as in mp_kmm_scan: different bases, or a text base outside
 * A/C/G/T) and a trailing run of at least `term` matching pairs, counted from the read's last base (as the text reads it) downwards
 * over aligned pairs: it ends at the first mismatch, ends at a deletion, and passes over inserted bases (an MD:Z tag does not show
 * them).  A site is reported once however many alignments reach it.  max_gap = 0 is the ungapped rule exactly.  Not covered: two
 * gaps in one alignment (bowtie2's default scoring admits them from L = 26 on) and gaps longer than MP_KMM_MAX_GAP. */
#define MP_KMM_GBAR 4
#define MP_KMM_MAX_GAP 4

/* mp_kmm_scan_resident (mprime.h) under the gapped rule: hits {sequence, start, pattern, strand} of the store of mp_seq_load, cap /
 * *n_hits as there.  MP_ERR_ARG when max_gap is outside 0 .. MP_KMM_MAX_GAP or max_penalty < 0. */
int mp_kmm_gap_scan_resident(struct mp_ctx *ctx, int32_t n_patterns, const uint8_t *pat_codes, const int32_t *pat_off, int32_t max_penalty,
                             int32_t max_gap, int32_t term, int64_t cap, int32_t *hits, int64_t *n_hits);

/* mp_offtarget_resident under the gapped rule: max_penalty[i] is read i's penalty ceiling (one launch per distinct ceiling); the site
 * reduction, the join, the kept products and mp_offtarget_stats are those of mp_offtarget_resident. */
int mp_offtarget_gap_resident(struct mp_ctx *ctx, int32_t n_patterns, const uint8_t *pat_codes, const int32_t *pat_off,
                              const int32_t *read_primer, const int32_t *max_penalty, int32_t max_gap, int32_t term, int32_t size_lo,
                              int32_t size_hi, int64_t cap, int32_t *out, int64_t *n_out);

/* Of the last mp_offtarget_resident / mp_offtarget_gap_resident / mp_amplicon_join of this context: ms[4] = {scan, site reduction, join, whole call} (device
 * event times of the first three stages; the whole call on the host clock, copies included) and counts[7] = {hits, forward sites,
 * reverse sites, products, sequences with forward sites, with reverse sites, with both}.  A call served from the kept products
 * reports zero device times and the counts of the call that made them. */
int mp_offtarget_stats(struct mp_ctx *ctx, double *ms, int64_t *counts);

#ifdef __cplusplus
}
#endif

#endif
