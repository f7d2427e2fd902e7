/*
 * mprime_ont.h — C ABI of assigning amplicon read ends to primers: the step the reference runs as FindONTprimerV3.py /
 * FindONTexpandprimer.py, whose cost is (reads x 2 ends) x (expanded primers x 2 strands) calls of difflib.SequenceMatcher.ratio().
 * multiprime_amd/csrc/ont.hip; exported by libmprime_hip.so only (the checker of these calls is the plain restatement of the rule
 * below in tests/ont_ref.py, beside difflib itself).  Conventions as in mprime.h: MP_OK (0) or a negative MP_ERR_* code, the message
 * in mp_last_error(ctx); the caller owns every buffer.  The host side (key list, pieces, names, tally) is multiprime_amd/ontprimer.py.
 *
 * THE RULE
 *
 * A PIECE is one end of a read, a KEY one expanded primer or its reverse complement; both are byte strings of 0 .. MP_ONT_MAX_LEN
 * bytes.  difflib's ratio of (piece a, key b) is 2 M / T with T = len(a) + len(b) (1.0 when T = 0) and M the Ratcliff/Obershelp match
 * count.  Nothing is junk and autojunk only acts from 200 characters, so M(a, b) is:
 *     1. keep a stack of ranges (alo, ahi, blo, bhi), starting with the whole strings (nothing if either is empty);
 *     2. pop a range;
 *     3. find the longest common substring a[i .. i+k) = b[j .. j+k) inside it; among equals the smallest i, then the smallest j;
 *     4. add k to M;
 *     5. if k > 0 push (alo, i, blo, j) and (i+k, ahi, j+k, bhi), each only where both sides are non-empty.
 * The order in which pending ranges are taken does not change the sum.
 *
 * The winner of a piece is decided on integers.  The caller passes a table q[T][M] (MP_ONT_Q_ROWS x MP_ONT_Q_COLS, int32) that ranks
 * the values its own arithmetic gives for (M, T) — for the drop-in: round(2.0 * M / T, 2) as Python evaluates it, equal floats equal
 * ranks — and the device keeps, per piece, the key with the larger q and on equal q the smaller index: "the maximum, and the first
 * index that reaches it" of the reference.  The call returns that key's index and its M; the caller turns (M, T) back into its
 * number.  No floating point runs on the device.  q must not decrease along M in any row (0 <= q < 65536): MP_ERR_ARG otherwise.
 *
 * LIMITS, refused with MP_ERR_ARG before anything is launched
 *     a key or a piece longer than MP_ONT_MAX_LEN (64) bytes — the key or piece is named;
 *     a key byte other than upper-case A, C, G, T — the key and the byte are named.  A piece may hold any byte: one that is none of
 *       the four (N, lower case, the newline the reference leaves at the end of a plain-text line) matches no key byte, which is what
 *       the reference's byte comparison does with such keys;
 *     no keys, or more than MP_ONT_MAX_KEYS of them;
 *     mp_ont_assign before mp_ont_set_keys.
 *
 * HOW IT RUNS (results do not depend on any of it)
 *
 * One lane owns one piece, held as four position masks (A, C, G, T) in registers: 64-bit words, or 32-bit words in a launch where no
 * piece and no key has more than 32 bytes (MP_ONT_WORD=64 keeps 64-bit words; the results are the same).  Keys are wave-uniform:
 * length, base counts and four position masks each, read through uniform loads; every lane walks the keys of its workgroup in
 * ascending order and keeps its own best.  Diagonal d of the match matrix is OR_c (piece_mask[c] & shift(key_mask[c], d)), clipped to
 * the range; the longest run of ones in that word is the diagonal's candidate.  The range stack (MP_ONT_STACK entries of four bytes, 17
 * on 32-bit masks) is one LDS column per lane.
 * A key whose composition bound  M <= sum_c min(count_a[c], count_b[c])  cannot reach a q above the lane's best is skipped
 * (MP_ONT_PRUNE=0 turns that off; the results are the same).  With few pieces the key list is split over workgroups
 * (MP_ONT_KEYS_PER_BLOCK=<keys> sets the split size, read per call); a workgroup leaves its best per piece with one 64-bit atomicMax
 * of  q << 40 | (0xFFFFFFFF - key) << 8 | M.
 */
#ifndef MPRIME_ONT_H
#define MPRIME_ONT_H

#include <stdint.h>

#include "mprime.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MP_ONT_MAX_LEN 64
#define MP_ONT_STACK 33                 /* pending ranges of one pair at the most: 2 t + 1 <= 64 letters for a chain of t matches */
#define MP_ONT_Q_ROWS 129               /* T = 0 .. 128 */
#define MP_ONT_Q_COLS 65                /* M = 0 .. 64 */
#define MP_ONT_MAX_KEYS (1 << 24)

/* Make n_keys keys resident — raw bytes back to back, key i = bytes[off[i] .. off[i+1]), an empty key is allowed.  Replaces a list set
 * before; a refused call leaves the earlier list in place. */
int mp_ont_set_keys(struct mp_ctx *ctx, int32_t n_keys, const uint8_t *bytes, const int64_t *off);

/* The winner of every piece against the resident keys: key[p] = its index, m[p] = its match count.  Pieces as the keys are given;
 * q as described above. */
int mp_ont_assign(struct mp_ctx *ctx, int64_t n_pieces, const uint8_t *bytes, const int64_t *off, const int32_t *q, int32_t *key, int32_t *m);

/* ms[1] = device event time of the assignment kernels since the last mp_ont_set_keys; counts[2] = {keys resident, pieces assigned since}. */
int mp_ont_stats(struct mp_ctx *ctx, double *ms, int64_t *counts);

#ifdef __cplusplus
}
#endif

#endif
