/*
 * mprime_ani.h — C ABI of merging rare clusters by average nucleotide identity: the step the pipeline runs as
 * merge_cluster_by_ANI.py, which calls `fastANI --ql A.txt --rl B.txt` for every (rare cluster, larger cluster) combination.
 * multiprime_amd/csrc/ani.hip; exported by libmprime_hip.so only (the checker of these calls is the plain restatement of the rule
 * below in tests/ani_ref.py).  Conventions as in mprime.h: MP_OK (0) or a negative MP_ERR_* code, the message in mp_last_error(ctx);
 * the caller owns every buffer.  fastANI's numbers cannot be reproduced without the binary; what is delivered is the deterministic,
 * integer-only rule stated here.  The host-side decisions (multiprime_amd/animerge.py) are pinned to the reference script itself.
 *
 * THE RULE
 *
 * Words and hash.  Letters are upper-cased (base_code of csrc/seedword.hpp).  A word is 12 consecutive letters, all in A/C/G/T; its
 * value is the 24-bit number with the first letter most significant (A = 0, C = 1, G = 2, T = 3), as seed_word of csrc/seedword.hpp
 * builds it.  Its hash is murmur3's 32-bit finaliser of that value:
 *     h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16        (mod 2^32)
 * The finaliser is a bijection, so distinct words have distinct hashes.  (0xFFFFFFFF is the hash of 0x331DA083, which is no 24-bit
 * value: no word hashes to it, and the library uses it for "no entry".)
 *
 * Sketch.  The sketch of a sequence at size s (MP_ANI_MIN_SKETCH .. MP_ANI_MAX_SKETCH, default 1024) is the s smallest distinct
 * hashes of its words, ascending; if the sequence has fewer than s distinct words, all of them.  A sketch of exactly s entries is
 * FULL.  A sequence shorter than 12 letters, or without a valid word, has an empty sketch.
 *
 * A pair (A, B) of sketches.
 *     c        the smallest last element among the full sketches of the two; if neither is full there is no limit
 *     w        |{x in A and in B, x <= c}|
 *     u        |{x in A, x <= c}| + |{x in B, x <= c}| - w
 *     jq       (w * 1024) / u in integers, 0 when u = 0
 *     ani_ppm  TAB[jq]
 * Below c both sketches list every hash of their sequences, so w / u is the Jaccard index of the two word sets up to c.  (An element
 * of both sketches is never above c.)
 *
 * TAB[0 .. 1024].  TAB[0] = 0; otherwise, with j = q / 1024.0 in double,
 *     TAB[q] = max(0, floor(1e6 * (1 + ln(2 j / (1 + j)) / 12) + 0.5))
 * — the Mash identity for k = 12, in parts per million.  The library computes the table once on the host (mp_ani_table exports it);
 * no floating point runs on the device.
 *
 * Reported.  A pair is reported iff ani_ppm >= report_ppm (the tools' default floor is 0.7, the minimum the reference's help text
 * names for -a).
 *
 * Two groups (P, R) of sequences.  n_rep is the number of reported pairs over all (p in P, r in R); sum_ppm is the sum of their
 * ani_ppm (int64).  A cluster merges into another on these two numbers: n_rep > 0 and sum_ppm >= ani_ppm_threshold * n_rep, i.e.
 * the mean identity of the reported pairs reaches the threshold — in integers.
 *
 * Limits, refused with MP_ERR_ARG before anything is launched: a record longer than MP_ANCHOR_MAX_LEN (32767) bases, the limit of the
 * step that made the clusters (the record is named); s outside 16 .. 1024; report_ppm outside 0 .. 1000000; an index or a group
 * outside the resident set.
 *
 * Not attempted: several GPUs.
 *
 * THE RULE, BOTH STRANDS (mp_ani_sketch_strands; off unless asked for — the rule above stays the rule of mp_ani_sketch)
 *
 * Canonical value.  A word has its forward value f as above.  Its reverse-complement word (the word reversed, A <-> T, C <-> G) has
 * the value r.  The canonical value is cv = min(f, r).  An occurrence of a word is AS READ iff f == cv; a palindromic word (f == r)
 * is always as read.
 *
 * Hash.  fmix32(cv).  cv is still a 24-bit value, so distinct canonical values have distinct hashes and none is 0xFFFFFFFF.
 *
 * Canonical sketch at size s.  The s smallest distinct hashes of the record's canonical values, ascending; FULL and empty as above.
 *
 * Orientation bit of a sketch element.  0 if the record holds at least one as-read occurrence of that canonical word, otherwise 1.
 * (The canonical sketch of the reverse complement of a record has the same hashes; every bit is flipped but those of palindromic
 * words and of words the record holds in both orientations, which are 0 on both sides.)
 *
 * A pair (A, B).  c, w, u, jq and ani_ppm exactly as above, on the canonical sketches.  In addition
 *     same     the number of shared elements <= c whose two orientation bits are equal
 *     opp      w - same
 *
 * Two groups (P, R).  n_rep and sum_ppm as above.  SAME and OPP are the sums of same and opp over the REPORTED pairs only.  The
 * strand of P against R is '-' iff OPP > SAME, otherwise '+' (a tie, 0 / 0 included, is '+').
 *
 * HOW IT RUNS (results do not depend on any of it)
 *
 * mp_ani_sketch: one workgroup per sequence hashes every word into LDS, sorts them there (bitonic, in one of five sizes by the
 * sequence's word count: 256, 2048, 8192, 16384 or 32768 keys, the last 128 KiB of the CU's 160 KiB), and writes the first s
 * distinct keys.  mp_ani_groups: a workgroup stages a tile of 8 sketches of the query group in LDS; its four wavefronts walk a chunk
 * of 64 sketches of the other group, each held in a wave's registers (entry i in lane i mod 64); a pair is 64 binary searches abreast
 * into the LDS sketch; (n_rep, sum_ppm) are summed per wave in registers and leave the workgroup as one 64-bit atomic add per
 * output.  Integers make the order of those additions irrelevant.  A launch stays below the runtime's limit of 2^32 work-items: more
 * work than that goes out as several launches that add into the same outputs (MP_ANI_MAX_GRID=<workgroups> lowers the cap, read per
 * call).
 *
 * mp_ani_sketch_strands: the same kernel in a second form.  A lane rolls the reverse-complement word beside the forward one (primed
 * over the same 11 letters, valid with it) and hashes the smaller; sort and compaction are the forward form's, and the compacted
 * sketch also stays in 4 KiB of LDS.  Then every lane walks its positions once more, looks the hash of each as-read occurrence up in
 * that sketch and sets a bit in a 128-byte LDS array; the complement goes out.  The comparison kernels run on a canonical set as
 * they are.  mp_ani_pairs_strand is one wave per pair on the pair layout (first sketch and its bit words in the wave's LDS slice,
 * the second in registers); mp_ani_groups_strand runs the group kernel's work list once more over the few decided group pairs.
 */
#ifndef MPRIME_ANI_H
#define MPRIME_ANI_H

#include <stdint.h>

#include "mprime_anchor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MP_ANI_WORD 12
#define MP_ANI_MIN_SKETCH 16
#define MP_ANI_MAX_SKETCH 1024
#define MP_ANI_TABLE 1025              /* entries of TAB */
#define MP_ANI_PAIR 3                  /* int32 per pair record: w, u, ani_ppm */
#define MP_ANI_PPM 1000000

/* Build the sketches of n sequences at size s and keep them resident — raw bytes back to back, sequence i = bytes[off[i] .. off[i+1]),
 * any letter case, a record may be empty.  The sequences themselves need not stay.  Replaces a set sketched before. */
int mp_ani_sketch(struct mp_ctx *ctx, int32_t n, const uint8_t *bytes, const int64_t *off, int32_t s);

/* The resident sketches: hashes[n * s] (sketch i at hashes + i * s, ascending, 0xFFFFFFFF past its size) and sizes[n]. */
int mp_ani_sketches(struct mp_ctx *ctx, uint32_t *hashes, int32_t *sizes);

/* (w, u, ani_ppm) of n_pairs pairs of resident sketches: out[n_pairs][MP_ANI_PAIR].  The unit of the rule. */
int mp_ani_pairs(struct mp_ctx *ctx, int64_t n_pairs, const int32_t *a_idx, const int32_t *b_idx, int32_t *out);

/* Groups are contiguous ranges of the resident sequences: group g = [group_off[g], group_off[g+1]).  For n_gp pairs of groups
 * (q_group[x], r_group[x]): out[x] = {n_rep, sum_ppm} over all (p in the first, r in the second) at the floor report_ppm. */
int mp_ani_groups(struct mp_ctx *ctx, int32_t n_groups, const int32_t *group_off, int64_t n_gp, const int32_t *q_group, const int32_t *r_group,
                  int32_t report_ppm, int64_t *out);

/* TAB: out[MP_ANI_TABLE].  Needs no context and no device. */
int mp_ani_table(int32_t *out);

/* ms[2] = {sketching (the last mp_ani_sketch), comparison (summed over the mp_ani_pairs / mp_ani_groups calls since)}: device event
 * times; counts[2] = {sketches resident, sequence pairs compared since the last mp_ani_sketch}. */
int mp_ani_stats(struct mp_ctx *ctx, double *ms, int64_t *counts);

/* ---- both strands (THE RULE, BOTH STRANDS) ---- */
#define MP_ANI_OR_WORDS(s) (((s) + 31) / 32)   /* uint32 per sketch of orientation bits */

/* mp_ani_sketch with canonical sketches and their orientation bits; arguments, refusals and replacement of the resident set as there.
 * mp_ani_sketches, mp_ani_pairs, mp_ani_groups and mp_ani_stats serve a canonical set as they serve a forward one. */
int mp_ani_sketch_strands(struct mp_ctx *ctx, int32_t n, const uint8_t *bytes, const int64_t *off, int32_t s);

/* The orientation bits of the resident canonical set: bits[n][MP_ANI_OR_WORDS(s)], bit i % 32 of word i / 32 is entry i of the
 * sketch; bits past a sketch's size are zero. */
int mp_ani_orientations(struct mp_ctx *ctx, uint32_t *bits);

/* (same, opp) of n_pairs pairs of resident canonical sketches: out[n_pairs][2].  The unit of the strand rule. */
int mp_ani_pairs_strand(struct mp_ctx *ctx, int64_t n_pairs, const int32_t *a_idx, const int32_t *b_idx, int32_t *out);

/* Groups and group pairs as in mp_ani_groups: out[x] = {SAME, OPP} over the pairs reported at the floor report_ppm. */
int mp_ani_groups_strand(struct mp_ctx *ctx, int32_t n_groups, const int32_t *group_off, int64_t n_gp, const int32_t *q_group,
                         const int32_t *r_group, int32_t report_ppm, int64_t *out);

/* mp_ani_orientations, mp_ani_pairs_strand and mp_ani_groups_strand return MP_ERR_ARG, with a message, when the resident set is a
 * forward one (mp_ani_sketch); their other argument checks are those of mp_ani_pairs and mp_ani_groups. */

#ifdef __cplusplus
}
#endif

#endif
