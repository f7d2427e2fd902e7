/*
 * mprime_anchor.h — C ABI of anchored alignment: unaligned sequences are placed on the columns of a small seed alignment, keeping
 * the seed's width (what `mafft --addfragments --keeplength` does on a CPU).  multiprime_amd/csrc/anchor.hip; exported by
 * libmprime_hip.so only (the oracle library serves mprime.h; the checker of these calls is the plain restatement of the rule below
 * in tests/anchor_ref.py).  Conventions as in mprime.h: MP_OK (0) or a negative MP_ERR_* code, the message in mp_last_error(ctx);
 * the caller owns every buffer.
 *
 * THE RULE
 *
 * Anchor.  From the seed alignment (R rows x L columns, letters upper-cased): column c is an anchor column when strictly more than
 * R / 2 rows hold a non-gap letter there (2 * rows > R); its anchor base is the most frequent of A, C, G, T in the column, ties to
 * the earlier letter in the order A, C, G, T, and `N` when no row holds A/C/G/T there.  The anchor sequence a (length n) is the
 * anchor bases in column order, col[j] the seed column of anchor position j.  An unaligned one-record FASTA is the R = 1 case.  This
 * step is tiny and is the caller's (multiprime_amd/anchor.py: anchor_of): mp_anchor_set takes a and col.
 *
 * Pair score of a query base q[i] and an anchor base a[j] (the query upper-cased): +match when both are the same letter of
 * A/C/G/T, -mismatch when both are A/C/G/T and differ, 0 when either is anything else.  A gap of g positions costs
 * open + g * extend.  Defaults: match 5, mismatch 4, open 10, extend 2; non-negative, at most MP_ANCHOR_MAX_PARAM each.
 *
 * Shape.  The whole query (length m) is aligned; anchor positions before its first and after its last aligned base are free.  With
 * cells (i, j), 0 <= i <= m query bases and 0 <= j <= n anchor positions consumed, and three states per cell (Gotoh):
 *     H(0, j) = 0, E(0, j) = F(0, j) = -inf
 *     E(i, j) = max(H(i, j-1) - open - extend  [the gap opened here],  E(i, j-1) - extend  [the gap extends])
 *               the alignment ends with an anchor column opposite no query base (a deletion: charged)
 *     F(i, j) = max(H(i-1, j) - open - extend  [opened],               F(i-1, j) - extend  [extends])
 *               the alignment ends with a query base opposite no anchor column (an insertion: charged, also at the query's ends)
 *     H(i, j) = max(H(i-1, j-1) + score(q[i-1], a[j-1]),  E(i, j),  F(i, j))            for i >= 1
 * where a term whose predecessor cell does not exist is -inf.  The end cell is the j that maximises H(m, j) inside the band, ties to
 * the smallest j.
 *
 * Band.  Only cells with d = j - i in [d0 - W, d0 + W] exist (W: params.band, 0 .. MP_ANCHOR_MAX_BAND).  d0 is the seed diagonal:
 * every pair (i, j) with q[i .. i+12) == a[j .. j+12), all 24 letters in A/C/G/T, casts one vote for j - i; d0 is the diagonal with
 * the most votes, ties to the smallest |d|, then to the smaller d; with no vote d0 = 0, clamped into [-m, n].  When the band admits
 * no path from row 0 to row m (H(m, j) = -inf throughout: a band that lies wholly left of diagonal 0, for instance) the query has no
 * alignment: score MP_ANCHOR_NO_SCORE, an all-gap row, no ops, zero counts, columns -1, status 3.
 *
 * Traceback from the end cell: in H prefer the diagonal move, then E, then F; in E and in F prefer "the gap opened here" over "the
 * gap extends" when both give the stored value.  It stops in state H on row 0.
 *
 * Outputs per query: the row (L bytes, '-' everywhere except row[col[j]] = the query's own upper-cased letter, whatever it is, for
 * every aligned pair; inserted bases are dropped, which keeps the length) and the meta record below.
 *     status bit 0   n_match * 1000 < min_identity_permille * m: the row is not part of the alignment (the caller drops it)
 *     status bit 1   a cell of the chosen path (its row-0 start and its end cell included) lies on diagonal d0 - W or d0 + W:
 *                    a warning to rerun with a wider band; the row is still written
 * On request the op string over M (pair), D (anchor column skipped), I (query base dropped), first to last aligned position:
 * m + n_del letters.
 *
 * Limits: query and anchor length 1 .. MP_ANCHOR_MAX_LEN each; scores are int32.  A seed alignment from nothing and an
 * anchor re-estimated from the added rows are mprime_star.h's.  Not attempted: several GPUs.
 *
 * ORIENTATION (both strands; off unless mp_anchor_strands(ctx, 1) was called).  rc(s) is the upper-cased record reversed, each letter
 * mapped A<>T, C<>G, R<>Y, K<>M, B<>V, D<>H, U->A; S, W, N and any other byte stay as they are.  Let (c+, d+) be the vote count and the
 * diagonal of the best diagonal of the votes of q against the anchor, exactly as above, and (c-, d-) the same for rc(q).  The query
 * is turned iff c- > c+, strictly: equal counts — no vote at all, a query under 12 bases, a query that is its own reverse complement
 * — leave it as it stands.  From there on the query IS rc(q): d0, the alignment, the row's letters, the ops and the counts are those
 * of the rule above applied to the oriented record.
 *     status bit 3   (MP_ANCHOR_REVERSED) the row is that of the reverse complement of the input record
 * (bit 2 is internal and never set in a record handed back.)
 */
#ifndef MPRIME_ANCHOR_H
#define MPRIME_ANCHOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct mp_ctx;

#define MP_ANCHOR_MAX_LEN 32767        /* query bases / anchor positions */
#define MP_ANCHOR_MAX_BAND 255         /* W: up to 511 diagonals, eight per lane of the query's wavefront */
#define MP_ANCHOR_MAX_PARAM 4095       /* match, mismatch, open, extend: (m + n) * (open + extend) stays below 2^29 */
#define MP_ANCHOR_WORD 12              /* letters of a vote word */
#define MP_ANCHOR_NO_SCORE INT32_MIN   /* the band admits no alignment */
#define MP_ANCHOR_META 10              /* int32 per meta record */
#define MP_ANCHOR_REVERSED 8           /* status bit 3: the reverse complement of the input record was aligned */

typedef struct mp_anchor_params {
    int32_t match, mismatch, gap_open, gap_extend;
    int32_t band;                      /* W */
    int32_t min_identity_permille;     /* 0 .. 1000 */
} mp_anchor_params;

/* One meta record per query (MP_ANCHOR_META int32). */
typedef struct mp_anchor_meta {
    int32_t score, d0, n_match, n_ins, n_del;
    int32_t first_col, last_col;       /* first / last seed column holding a base of the query; -1: none */
    int32_t status;
    int32_t first_anchor, last_anchor; /* the same two as anchor positions */
} mp_anchor_meta;

/* Keep the anchor in the context: anchor_codes[n] upper-case letters (A/C/G/T, anything else scores 0), col[n] strictly ascending
 * seed columns in [0, L).  Builds the lookup of the anchor's 12-mers (an open-addressing table of positions, built here and
 * uploaded once).  Replaces an anchor set before. */
int mp_anchor_set(struct mp_ctx *ctx, const uint8_t *anchor_codes, int32_t n, const int32_t *col, int32_t L,
                  const mp_anchor_params *params);

/* Align n_queries queries — raw bytes back to back, query q = bytes[off[q] .. off[q+1]), any letter case — to the anchor:
 * rows_out [n_queries][L] bytes, meta_out [n_queries] records.  want_ops != 0: ops_out receives the op strings, query q's RIGHT-
 * aligned in its slot [ops_off[q], ops_off[q+1]) (it ends at ops_off[q+1] and is m + n_del letters long); a slot holds at least
 * m + n bytes.  Queries run in batches sized so that the traceback bits (4 per cell) stay within a quarter of the free device
 * memory; MP_ANCHOR_BATCH=<queries>, read per call, caps the batch.  Results do not depend on the batching.  MP_ERR_ARG names the
 * first empty or over-long query; nothing is launched then. */
int mp_anchor_align(struct mp_ctx *ctx, int32_t n_queries, const uint8_t *bytes, const int64_t *off, int32_t want_ops,
                    uint8_t *rows_out, int32_t *meta_out, uint8_t *ops_out, const int64_t *ops_off);

/* A switch of the context, read by mp_anchor_align and by mp_star_round (mprime_star.h): both != 0 votes both strands of every query
 * and turns it as ORIENTATION says; 0 (the default) is the forward-only rule, with the kernels and results of before the switch existed. */
int mp_anchor_strands(struct mp_ctx *ctx, int32_t both);

/* Of the last mp_anchor_align of this context: ms[5] = {vote, DP, traceback + emit (device event times, summed over the batches),
 * read-back, whole call (host clock)}, counts[3] = {batches, DP cells, bytes of traceback bits of the largest batch}. */
int mp_anchor_stats(struct mp_ctx *ctx, double *ms, int64_t *counts);

#ifdef __cplusplus
}
#endif

#endif
