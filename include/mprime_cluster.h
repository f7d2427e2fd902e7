/*
 * mprime_cluster.h — C ABI of clustering by identity: greedy incremental clustering of unaligned sequences, the step the pipeline
 * runs as `cd-hit -c 1` (duplicate removal) and `cd-hit -c <identity>` (rule cluster_by_identity).  multiprime_amd/csrc/cluster.hip;
 * exported by libmprime_hip.so only (the checker of these calls is the plain restatement of the rule below in tests/cluster_ref.py).
 * Conventions as in mprime.h: MP_OK (0) or a negative MP_ERR_* code, the message in mp_last_error(ctx); the caller owns every buffer.
 * cd-hit's word filter is statistical and its output cannot be reproduced; what is delivered is the deterministic rule stated here.
 *
 * THE RULE
 *
 * Order.  Records are upper-cased; the id is the header's first token.  Sequences are processed by length descending, ties by input
 * order.
 *
 * Greedy.  In that order a sequence s joins the EARLIEST-CREATED representative r for which similar(s, r) holds (cd-hit's default:
 * first hit, not best hit).  If there is none it becomes a new representative; its cluster number is the count of representatives
 * before it.
 *
 * similar(s, r), with m = len(s) <= n = len(r):
 *   1. Seed.  The diagonal votes of mprime_anchor.h with s as the query and r as the anchor: every pair (i, j) with
 *      s[i .. i+12) == r[j .. j+12), all 24 letters in A/C/G/T, casts one vote for d = j - i; d0 is the diagonal with the most votes,
 *      ties to the smallest |d|, then to the smaller d; `votes` is the count on d0.  With votes < min_votes (default 1) the pair is
 *      not similar and no alignment is made.  A sequence shorter than 12 bases therefore always founds its own cluster.  (With
 *      min_votes = 0 every pair is aligned; without a vote d0 = 0.)
 *   2. Alignment.  Exactly the anchored-alignment recurrence of mprime_anchor.h with r as the anchor (col[j] = j) and s as the query:
 *      the whole of s is aligned, r's ends are free, band [d0 - W, d0 + W], the same pair scores with the same defaults (match 5,
 *      mismatch 4, open 10, extend 2), the same traceback preferences, the end cell the smallest j of the maximum.  n_match is what
 *      mp_anchor_align reports for that pair: the aligned pairs of equal letters of A/C/G/T on the traced path.
 *   3. Decision.  Similar iff a path exists and n_match * 1000 >= identity_permille * m.  Integers only; identity is over the shorter
 *      sequence, as cd-hit's default global identity.
 *
 * Reported identity of a member: (n_match * 10000 + m / 2) / m in integer arithmetic, printed as dd.dd%.
 *
 * Limits, refused with MP_ERR_ARG naming the first offending record before anything is launched: lengths 1 .. MP_ANCHOR_MAX_LEN;
 * band 0 .. MP_ANCHOR_MAX_BAND; match, mismatch, open, extend 0 .. MP_ANCHOR_MAX_PARAM; identity_permille 0 .. 1000; min_votes
 * 0 .. MP_ANCHOR_MAX_LEN.  A record whose 12-mers recur so often in a block of representatives that its vote table exceeds the
 * device budget (low-complexity repeats by the hundred thousand) is refused by name with MP_ERR_CAPACITY.
 *
 * BOTH STRANDS (mp_cluster_greedy_strands, mp_cluster_pairs_strands; what cd-hit-est does with -r 1).  rc(s) is mprime_anchor.h's: the
 * record reversed and complemented; in the code store a code below 4 (A, C, G, T = 0 .. 3) becomes 3 - code and every other code
 * stays.  similar+-(s, r): similar(s, r) is tested first and, if it holds, the strand is `+`; otherwise similar(rc(s), r) is tested
 * and, if it holds, the strand is `-`.  A sequence joins the earliest-created representative for which either test holds; a
 * representative always keeps its given orientation; n_match and the printed identity come from the strand that held.  Printed as
 * `at +/dd.dd%` and `at -/dd.dd%`.  The forward-only calls are untouched by this.
 *
 * Not attempted: best-hit mode (cd-hit -g 1), several GPUs.  A letter outside A/C/G/T never counts as a match, so at identity 1.0 a record containing N only ever founds its own cluster.
 *
 * HOW IT RUNS (results do not depend on any of it)
 *
 * The greedy loop runs in rounds over a block of the next B unassigned sequences in order.  Per round: (1) the block's members are
 * seeded and aligned against earlier members of the same block; (2) the host resolves in order which members are real
 * representatives — a member is one iff no earlier real representative of the block is similar to it; (3) every later unassigned
 * sequence is seeded and aligned against the block's real representatives; (4) it joins the smallest-numbered one that passes.
 * This equals the sequential rule for every B.  B is sized from free device memory (at most MP_CLUSTER_MAX_BLOCK);
 * MP_CLUSTER_BLOCK=<sequences> caps it and MP_CLUSTER_PAIR_BATCH=<pairs> caps the pairs of one alignment launch, both read per call.
 * Both strands: the first both-strand call builds rc of every resident sequence on the device as sequence n + i of the same store
 * (nothing is uploaded again; the store doubles until the next mp_cluster_load).  A seeding's queries are the forward copies and the
 * reverse copies; the reverse copy of a pair is aligned only where the forward test of that pair did not hold.
 */
#ifndef MPRIME_CLUSTER_H
#define MPRIME_CLUSTER_H

#include <stdint.h>

#include "mprime_anchor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MP_CLUSTER_MAX_BLOCK 32768     /* members of one block: a member number takes 15 bits of a vote key */
#define MP_CLUSTER_PAIR 5              /* int32 per pair record */
#define MP_CLUSTER_NOT_SEEDED 4        /* status bit 2: votes < min_votes, no alignment was made */

typedef struct mp_cluster_params {
    int32_t match, mismatch, gap_open, gap_extend;
    int32_t band;                      /* W */
    int32_t identity_permille;         /* 0 .. 1000 */
    int32_t min_votes;
} mp_cluster_params;

/* One record per pair (MP_CLUSTER_PAIR int32).  status bit 0: n_match * 1000 < identity_permille * m (not similar); bit 1: the path
 * touches diagonal d0 - W or d0 + W, as in mprime_anchor.h (both set, score MP_ANCHOR_NO_SCORE: the band admits no path); bit 2: not
 * seeded (score MP_ANCHOR_NO_SCORE, n_match 0, bit 0 set as well). */
typedef struct mp_cluster_pair {
    int32_t votes, d0, score, n_match, status;
} mp_cluster_pair;

/* Make n sequences resident — raw bytes back to back, sequence i = bytes[off[i] .. off[i+1]), any letter case.  Replaces a set
 * loaded before.  MP_ERR_ARG names the first empty or over-long record. */
int mp_cluster_load(struct mp_ctx *ctx, int32_t n, const uint8_t *bytes, const int64_t *off);

/* similar()'s numbers for n_pairs pairs of resident sequences, q_idx[p] the query and r_idx[p] the anchor (any two, also q longer
 * than r): out[n_pairs] records.  The unit the greedy loop is made of, and the all-against-representative identities on its own. */
int mp_cluster_pairs(struct mp_ctx *ctx, int64_t n_pairs, const int32_t *q_idx, const int32_t *r_idx, const mp_cluster_params *params,
                     int32_t *out);

/* The clustering of the resident sequences: cluster_of[n] the cluster number of every sequence, rep_of_cluster[n_clusters] (room for
 * n) the sequence that founded a cluster, n_match_of[n] a member's n_match against its representative (a representative: its own
 * length). */
int mp_cluster_greedy(struct mp_ctx *ctx, const mp_cluster_params *params, int32_t *cluster_of, int32_t *rep_of_cluster,
                      int32_t *n_match_of, int32_t *n_clusters);

/* mp_cluster_pairs with a strand per pair: q_strand[p] = 0 takes sequence q_idx[p] as the query, 1 takes rc of it; the anchor is
 * always the sequence as given.  Records as in mp_cluster_pairs. */
int mp_cluster_pairs_strands(struct mp_ctx *ctx, int64_t n_pairs, const int32_t *q_idx, const int32_t *r_idx, const int32_t *q_strand,
                             const mp_cluster_params *params, int32_t *out);

/* mp_cluster_greedy under BOTH STRANDS: strand_of[n] is 0 for a representative and for a member that joined as given, 1 for a member
 * whose reverse complement joined (n_match_of is that strand's). */
int mp_cluster_greedy_strands(struct mp_ctx *ctx, const mp_cluster_params *params, int32_t *cluster_of, int32_t *rep_of_cluster,
                              int32_t *n_match_of, int32_t *strand_of, int32_t *n_clusters);

/* Of the last mp_cluster_greedy / mp_cluster_pairs of this context: ms[5] = {block index, seed, alignment (device event times, summed
 * over the launches), host resolve, whole call (host clock)}, counts[3] = {rounds, candidate pairs aligned, DP cells}. */
int mp_cluster_stats(struct mp_ctx *ctx, double *ms, int64_t *counts);

#ifdef __cplusplus
}
#endif

#endif
