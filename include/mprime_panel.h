/*
 * mprime_panel.h — C ABI of the panel update (scripts/Primer_set_update.py, cited as PU by line): which NEW primers form 3'-end dimers
 * with a validated CORE set, and which core/new or new/new combinations of 3' terms amplify something in a background.  Exported by
 * libmprime_hip.so only (the oracle library serves mprime.h); mp_dimer_cross lives in multiprime_amd/csrc/dimer.hip beside the search
 * it shares, the class joins in multiprime_amd/csrc/offtarget.hip.  The checker of these calls is the plain restatement of the rule in
 * tests/panel_ref.py, itself pinned to what the unmodified reference writes (tests/golden/panel/, make_golden_panel.py).
 *
 * Conventions as in mprime.h: MP_OK (0) or a negative MP_ERR_* code, the message in mp_last_error(ctx); the caller owns every buffer.
 *
 * ---- THE RULE -------------------------------------------------------------------------------------------------------------------------
 * Primer files (PU:221-238).  FASTA read line by line: a line starting with '>' is a name (kept with its '>'); every other line, stripped,
 *   is a sequence keyed to the last name seen.  A sequence repeated inside one file keeps its FIRST position and its LAST name (a dict
 *   keyed by sequence).  The reference's .primer_set pickle caches beside the inputs are neither read nor written.
 * Sets (PU:179-192).  common = sequences of both files; uniq_new = new - common; uniq_core = core - common; merged = uniq_new + uniq_core +
 *   common, a common sequence named  new name + "|" + core name.
 * Dimer jobs (PU:287-294).  One job per core sequence in core-file order with partners uniq_new; then one job per new sequence in new-file
 *   order with partners merged.  A common sequence runs twice (once per file) and may print the same line twice; so does the reference.
 *   The printed Primer_ID of a job's primer is its name in merged; the partner's name is the one in the partner set walked.
 * Search per ordered pair x -> y (PU:258-285).  Ends of x: its 3' suffixes of length min(t, len x) for t = 18 .. 5, longest first, each
 *   length once, each expanded.  RC(end) is looked up with str.find in every expansion of y: the first occurrence counts, idx.
 *   d2 = len(y) - l - idx, GC = G + C of the end.  The pair is a hit at the FIRST (end, expansion of y) for which
 *       log10(2**l * 2**GC / ((0 + 0.1) * (d2 + 0.1))) > 3                    (PU:151-152; strict)
 *    or deltaG(end) < -5                                                     (PU:205-218; at ANY d2 — finDimer asks for d2 == 0)
 *   and gives one line per (job, partner) at most.  deltaG: the nearest-neighbour stack terms of finDimer, then ONE term
 *   adjust_initiation[first base] (2.8 for A/T, 1.82 for C/G) (+ 0.4 if the end's last two letters are "TA") + 0.4, evaluated left to right;
 *   no Na+ term; rounded to 2 decimals.
 *   Order inside one end length: the reference walks list(set(ends)) — for a degenerate primer that order changes with PYTHONHASHSEED.
 *   HERE the ends of one length are tried in expansion order (itertools.product order, last degenerate position fastest, as mp_dimer_scan
 *   documents).  For primers without degenerate letters the reference's set of lines is deterministic and is reproduced exactly.
 * Floating point.  No Loss or deltaG decision is made with device arithmetic that could differ from CPython's: loss_hit[l][GC][d2] is a
 *   byte table the host builds with the reference's own expression (math.log10, strict > 3); dg_params is the layout of mp_dimer_scan
 *   with PU's one term in every [first][last][TA] initiation slot (the same for every `last`) and zeros in the Na+ and symmetry slots
 *   (adding 0.0 changes no double); dg_limit is the smallest double whose round(x, 2) is not below -5.  The device only ADDS these doubles
 *   in the reference's order.
 * Off-target sites.  Per class (0 core, 1 new), strand, sequence and position a site belongs to the LAST read that claims it — the largest
 *   read index of that class (PU:429-431 turns a list into a dict).  A position claimed by both classes is a site of each.
 * Joins, in this order: class 0 = core forward x new reverse, class 1 = new forward x core reverse, class 2 = new forward x new reverse
 *   (never core x core).  Each is PU:427-454 per sequence: starts and stops ascending; no product at all when
 *   stops[0] - starts[-1] > hi or stops[-1] - starts[0] < lo; for each start the stops from closest() (bisect_left of start + lo .. the last
 *   stop below start + hi, or the last stop of all when start + hi is beyond it); the FIRST start whose range is empty ends the sequence;
 *   lo < length < hi with length = stop - start + 1, and the walk of a start breaks once length exceeds hi.
 *   Line by line this IS validate.amplicons() (mprime_offtarget.h, V9:318-345): the same two early outs with the same operands, the same
 *   bisect_left bounds and the same "first > last" break; the inner `length > hi: break` and `lo < length < hi` are amplicons()'
 *   "stop <= start + hi - 2" cut and its "length > lo" test (a stop with length == hi is skipped by PU's elif and lies past amplicons()'
 *   cut; nothing after it can pass either, the stops ascend).  The device joins are therefore join_device of offtarget.hip, run per class.
 *   Sequences come out per join class in ascending row order.
 */
#ifndef MPRIME_PANEL_H
#define MPRIME_PANEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct mp_ctx;

/* The rectangular dimer search.  Primers as in mp_dimer_scan (codes / off, 1..MP_DIMER_MAX_LEN symbols; lists holding a primer of more
 * than 32 bases use the 64-bit planes).  jobs[3j..] = {x, y_lo, y_hi}: primer x against the partners y_lo <= y < y_hi (0 <= y_lo <= y_hi
 * <= n_primers; an empty range is allowed).  With the primers laid out [uniq_new | uniq_core | common] a core job's partners are
 * [0, n_uniq_new) and a new job's [0, n_primers).  End lengths are mode 0's.  loss_hit / dg_params / dg_limit as in mp_dimer_scan, with
 * the deltaG test applied at every d2.  A hit is six int32 {job, y, end length, end expansion, y expansion, idx}; hits arrive in no
 * particular order; cap / *n_hits as in mp_dimer_scan: *n_hits is exact, hits receives the first min(cap, *n_hits) records written. */
int mp_dimer_cross(struct mp_ctx *ctx, int32_t n_primers, const uint8_t *codes, const int32_t *off, int32_t n_jobs, const int32_t *jobs,
                   const uint8_t *loss_hit, const double *dg_params, double dg_limit, int64_t cap, int32_t *hits, int64_t *n_hits);

/* A product of the class joins is seven int32: {row, start, stop, forward read, reverse read, length, join class}. */

/* The three joins alone on explicit sites: sites[5i..] = {class (0 core, 1 new), strand (0 forward, 1 reverse), row >= 0, position >= 0,
 * read}, strictly ascending in (class, strand, row, position) — one read per site, as the reduction leaves it.  Products come out join
 * class 0, 1, 2, rows ascending inside a class.  Holds no state. */
int mp_amplicon_join_classes(struct mp_ctx *ctx, int64_t n_sites, const int32_t *sites, int32_t size_lo, int32_t size_hi, int64_t cap,
                             int32_t *out, int64_t *n_out);

/* mp_offtarget_resident with one more array: read_class[i] is 0 (core) or 1 (new).  One scan of the store of mp_seq_load per distinct
 * mismatch budget (mp_kmm_scan's rule with `term`), the hits reduced on the device to one read per (class, strand, sequence, position) —
 * the largest read index of that class, reported as read_id[i] —, then the three joins on the device.  cap / *n_out as above.  The
 * products of the last call are kept with the context: a call with the same arguments on the same store that found *n_out > cap the
 * first time copies them out the second time without scanning again (the store is reloaded or freed: they are dropped).  The plain
 * screen's kept products (mp_offtarget_resident) do not survive this call. */
int mp_offtarget_classes(struct mp_ctx *ctx, int32_t n_patterns, const uint8_t *pat_codes, const int32_t *pat_off, const int32_t *read_id,
                         const int32_t *read_class, const int32_t *max_mismatch, int32_t term, int32_t size_lo, int32_t size_hi,
                         int64_t cap, int32_t *out, int64_t *n_out);

/* mp_offtarget_stats (mprime_offtarget.h) reports these calls too: the stage times of the whole call, hits, and the sites / sequences /
 * products summed over the three joins. */

#ifdef __cplusplus
}
#endif

#endif
