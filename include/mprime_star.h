/*
 * mprime_star.h — C ABI of the star alignment: the records of a cluster are aligned from nothing (what `mafft --auto` does in the
 * reference workflow's alignment step), every inserted base kept.  multiprime_amd/csrc/star.hip around the kernels of
 * anchorcore.hpp; exported by libmprime_hip.so only.  The checker of these calls is the plain restatement of the rule below in
 * tests/star_ref.py.  Conventions as in mprime.h: MP_OK (0) or a negative MP_ERR_* code, the message in mp_last_error(ctx); the
 * caller owns every buffer.
 *
 * THE RULE
 *
 * Records.  Those of the FASTA front end of every drop-in (msa.read_records: the id is the header's first token).  Letters are
 * upper-cased; `-` and `.` inside a record are removed before anything else; what remains has 1 .. MP_ANCHOR_MAX_LEN letters — an
 * empty or longer record is refused by name before any launch.  N >= 1; with N = 1 the output is that record.  (Removing `-` and `.`
 * is the caller's: multiprime_amd/starmsa.py.  mp_star_load takes the records as they are to be aligned.)
 *
 * A round takes an anchor a of n letters and produces an alignment.
 *   1. Every record, the centre included, is aligned to a by the anchored-alignment rule of mprime_anchor.h, unchanged: the 12-mer
 *      diagonal vote, the band [d0 - W, d0 + W], the same scores, traceback preferences and status bits; col is the identity.
 *   2. Band escalation.  A record whose status has bit 1 (the path touches the band's edge) or equals 3 (no path) is aligned again at
 *      W' = min(2 W, 255), and again, until neither holds or W' = 255.  The last attempt stands and its W goes into the record's
 *      meta.  The vote is not repeated: only the band changes.  (W >= 1, or the band would never grow.)
 *   3. A record is PLACED when its final status has bit 0 clear and is not 3.  Unplaced records take no further part in the round.
 *   4. Slots.  An inserted base (op I) met when j anchor positions have been consumed lies in slot j, 0 <= j <= n.  A path has at most
 *      one run of I per slot.  ins[j] is the maximum over the placed records of their run length in slot j.
 *   5. Columns.  Width L' = n + sum(ins).  Anchor position j is column acol[j] = j + sum(ins[g], g <= j).  Slot g < n owns the columns
 *      [acol[g] - ins[g], acol[g]); slot n owns the last ins[n] columns.
 *   6. Row of a placed record: `-` everywhere; its own letter at acol[j] for every aligned pair (op M); its inserted letters in their
 *      slot's columns — the run before the record's first M / D op right-justified in its slot, every other run left-justified.
 *      Removing `-` from the row gives back the record exactly.
 *
 * Rounds.  Round 0's anchor is the longest record, ties to the earliest in the input.  After a round the next anchor is anchor_of
 * (mprime_anchor.h) of the placed rows of that round: a column is an anchor column when strictly more than half of the placed rows hold
 * a letter there; its base is the most frequent of A / C / G / T, ties to the earlier letter, `N` when none occurs.  The next round
 * aligns every record, those unplaced before included, to that anchor and builds its columns afresh from 4 - 6: a non-anchor column of
 * the previous round survives only as insertions.  K rounds, 1 .. MP_STAR_MAX_ROUNDS (default 2); the loop stops early when the new
 * anchor equals the one just used.  A consensus of more than MP_ANCHOR_MAX_LEN letters (or of none: no record placed) is an error.
 * The output is the last round's alignment.  The round loop is the caller's (multiprime_amd/starmsa.py): mp_star_round is one round,
 * and the column counts it leaves are all the next anchor needs.
 *
 * Both strands (mprime_anchor.h: ORIENTATION; on after mp_anchor_strands(ctx, 1)).  Every round votes both strands of each record AS
 * IT IS CURRENTLY HELD and turns it iff the reverse complement's best diagonal has strictly more votes; a record that is turned stays
 * turned for the later rounds (the resident bytes are rewritten once), and mp_star_load holds every record as given again.  Status
 * bit 3 (MP_ANCHOR_REVERSED) of a round's meta record is the record's parity against the loaded record.  Round 0's centre is the
 * longest record in its given orientation (the caller's choice of anchor).  Everything else of the rule applies to the oriented record.
 *
 * Not attempted: progressive / guide-tree alignment, several GPUs.
 */
#ifndef MPRIME_STAR_H
#define MPRIME_STAR_H

#include <stdint.h>

#include "mprime_anchor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MP_STAR_MAX_ROUNDS 8
#define MP_STAR_META (MP_ANCHOR_META + 1)   /* int32 per record: the mp_anchor_meta fields (columns = anchor positions), then the final W */
#define MP_STAR_COUNTS 6                     /* per column: A, C, G, T, any other letter, gap — over the placed rows */

/* The records become resident: record q = bytes[off[q] .. off[q+1]), any letter case, 1 .. MP_ANCHOR_MAX_LEN letters each
 * (MP_ERR_ARG names the first that is not; nothing is launched then).  Replaces records loaded before and drops their last round. */
int mp_star_load(struct mp_ctx *ctx, int32_t n_records, const uint8_t *bytes, const int64_t *off);

/* One round against anchor[n] (upper-case letters; anything but A/C/G/T scores 0).  params as in mp_anchor_set with band >= 1 (the
 * context's anchor of mp_anchor_set is replaced by this one).  meta_out [n_records][MP_STAR_META]; ins_out [n + 1]; *width_out = L'.
 * The rows [n_records][L'] (all-gap for unplaced records) and the column counts [L'][MP_STAR_COUNTS] stay on the device for
 * mp_star_rows / mp_star_counts, whose sizes the caller knows only now.  Records run in batches whose traceback bits (4 per cell)
 * stay within a quarter of the free device memory; MP_STAR_BATCH=<records>, read per call, caps a batch.  Results do not depend on
 * the batching.  The path store of a round (two uint16 per record and slot, beside the letters in anchor space) is sized for all
 * records: MP_ERR_CAPACITY with the byte count when the device cannot hold it. */
int mp_star_round(struct mp_ctx *ctx, const uint8_t *anchor, int32_t n, const mp_anchor_params *params, int32_t *meta_out,
                  int32_t *ins_out, int32_t *width_out);

/* Of the last round: rows_out [n_records][L'] / counts_out [L'][MP_STAR_COUNTS]. */
int mp_star_rows(struct mp_ctx *ctx, uint8_t *rows_out);
int mp_star_counts(struct mp_ctx *ctx, int32_t *counts_out);

/* Of the last mp_star_round: ms[8] = {vote, DP, traceback + path store + escalation lists, insertion profile + scan + column map, row
 * writer, column counts (device event times, summed over batches and band levels), read-back, whole call (host clock)}, counts[6] =
 * {batches, DP cells, records aligned again (summed over band levels), bytes of traceback bits held, bytes of the path store, placed}. */
int mp_star_stats(struct mp_ctx *ctx, double *ms, int64_t *counts);

/* Release the records and the last round. */
int mp_star_free(struct mp_ctx *ctx);

#ifdef __cplusplus
}
#endif

#endif
