// anchorcore.hpp — the device side of the anchored-alignment rule (include/mprime_anchor.h), shared by anchor.hip (one pass onto a seed's
// columns) and star.hip (rounds onto a re-estimated anchor, inserted bases kept).  Three kernels per batch of queries:
//   anchor_vote_kernel   one wavefront per query: its 12-mers (seedword.hpp) are looked up in the anchor's open-addressing table, the
//                        votes per diagonal counted in an LDS histogram (two 16-bit counters per word), d0 chosen by a wave reduction
//                        — one call of vote_pass, the only body of the histogram vote
//   anchor_orient_kernel its both-strand form (mp_anchor_strands): vote_pass over the same histogram for q and then for rc(q), the
//                        query's bytes rewritten in place as rc(q) where that seeds better; anchor_mark_kernel sets status bit 3 afterwards
//   anchor_dp_kernel     one wavefront per query: band_sweep (bandsweep.hpp: the recurrence, its comparison order and the end cell) with
//                        the TRACE payload — four predecessor bits per cell (H source 2, E opened, F opened) are collected eight rows
//                        to a word per diagonal and stored to the traceback buffer in HBM.  Anchor codes (shared by the workgroup's
//                        waves) and the wave's query codes sit in LDS, so no per-letter profile rows are kept.
//   anchor_trace_kernel  one lane per query walks the bits from the end cell (a chain of dependent loads: latency-bound, so it
//                        gets its parallelism from the number of queries), writes the letters in anchor space, the meta record and the ops
// Everything sits in an unnamed namespace: each translation unit that includes this compiles the kernels it instantiates.
#pragma once

#include "bandsweep.hpp"
#include "seedword.hpp"

namespace mp {

namespace {

// ---- votes --------------------------------------------------------------------------------------------------------------------------
// better(a, b): diagonal vote (ca, da) beats (cb, db) — more votes, then the smaller |d|, then the smaller d
__device__ inline bool vote_better(int ca, int da, int cb, int db) {
    if (ca != cb) return ca > cb;
    const int aa = da < 0 ? -da : da, ab = db < 0 ? -db : db;
    if (aa != ab) return aa < ab;
    return da < db;
}

// One pass of the vote over the wave's histogram hist[0 .. (m + n) / 2] (cleared on entry, all lanes): bin b = d + m (1 .. m + n - 1) is
// counter (b & 1) of word b >> 1.  kRev: over the words of rc(q), read from the forward bytes — the word of rc(q) at i' = m - 12 - i is the
// window q[i .. i + 12) with its letters complemented and their order reversed, so its bin is j - i' + m.  Returns the best (votes,
// diagonal) in every lane; votes 0: no vote.  A second pass over the same histogram needs a barrier first: lanes still read it here.
template <bool kRev>
__device__ inline void vote_pass(uint32_t *hist, const uint8_t *qb, int m, int n, const uint32_t *__restrict__ akmer,
                                 const int32_t *__restrict__ table, int log2_slots, int lane, int *best_c_out, int *best_d_out) {
    const int words = (m + n) / 2 + 1;
    for (int x = lane; x < words; x += 64) hist[x] = 0;
    __syncthreads();
    const uint32_t mask = (1u << log2_slots) - 1;
    for (int i = lane; i + kWord <= m && n >= kWord; i += 64) {
        const uint32_t kmer = kRev ? seed_word_rc_letters(qb + i) : seed_word_letters(qb + i);
        if (kmer == kEmpty) continue;
        const int iq = kRev ? m - kWord - i : i;
        uint32_t slot = word_hash(kmer, log2_slots);
        for (int32_t j; (j = table[slot]) >= 0; slot = (slot + 1) & mask)
            if (akmer[j] == kmer) {
                const int b = j - iq + m;
                atomicAdd(&hist[b >> 1], (b & 1) ? 65536u : 1u);
            }
    }
    __syncthreads();
    int best_c = 0, best_d = 0;
    for (int b = 1 + lane; b <= m + n - 1; b += 64) {
        const int cnt = (int)((hist[b >> 1] >> ((b & 1) * 16)) & 0xFFFFu);
        if (cnt > 0 && (best_c == 0 || vote_better(cnt, b - m, best_c, best_d))) { best_c = cnt; best_d = b - m; }
    }
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const int oc = __shfl_xor(best_c, sh), od = __shfl_xor(best_d, sh);
        if (oc > 0 && (best_c == 0 || vote_better(oc, od, best_c, best_d))) { best_c = oc; best_d = od; }
    }
    *best_c_out = best_c;
    *best_d_out = best_d;
}

__global__ __launch_bounds__(64) void anchor_vote_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ off, int n,
                                                          const uint32_t *__restrict__ akmer, const int32_t *__restrict__ table, int log2_slots,
                                                          int32_t *__restrict__ d0_out) {
    extern __shared__ uint32_t hist[];
    const int q = blockIdx.x, lane = threadIdx.x;
    const int m = (int)(off[q + 1] - off[q]);
    int best_c, best_d;
    vote_pass<false>(hist, bytes + off[q], m, n, akmer, table, log2_slots, lane, &best_c, &best_d);
    if (lane == 0) d0_out[q] = best_c > 0 ? best_d : min(max(0, -m), n);
}

// ---- both strands (mprime_anchor.h: ORIENTATION) -------------------------------------------------------------------------------------
// anchor_vote_kernel for both strands: one wavefront per query, the same histogram (up to (m + n) / 2 + 1 words) for the forward pass
// and then for the pass over rc(q).  The query is turned iff rc(q)'s best diagonal has strictly more votes; then the wave rewrites the
// query's bytes IN PLACE as rc(q) — lane x swaps the pair (x, m - 1 - x) through upper_letter and complement_letter, pairs are disjoint,
// an odd m's middle letter is complemented where it stands — and every kernel after this one reads the oriented record.  d0 is that of
// the record as it is left.  flag[q]: kToggle (star.hip's resident parity) ^= turned, else = turned.
template <bool kToggle>
__global__ __launch_bounds__(64) void anchor_orient_kernel(uint8_t *__restrict__ bytes, const int64_t *__restrict__ off, int n,
                                                            const uint32_t *__restrict__ akmer, const int32_t *__restrict__ table, int log2_slots,
                                                            int32_t *__restrict__ d0_out, uint8_t *__restrict__ flag) {
    extern __shared__ uint32_t hist[];
    const int q = blockIdx.x, lane = threadIdx.x;
    uint8_t *qb = bytes + off[q];
    const int m = (int)(off[q + 1] - off[q]);
    int cf, df, cr, dr;
    vote_pass<false>(hist, qb, m, n, akmer, table, log2_slots, lane, &cf, &df);
    __syncthreads();                           // (every lane has read the histogram before the next pass clears it)
    vote_pass<true>(hist, qb, m, n, akmer, table, log2_slots, lane, &cr, &dr);
    const bool turn = cr > cf;                 // (uniform over the wave: both reductions leave every lane with the same pair)
    if (turn) {
        for (int x = lane; x < m / 2; x += 64) {
            const uint8_t lo = qb[x], hi = qb[m - 1 - x];
            qb[x] = complement_letter(upper_letter(hi));
            qb[m - 1 - x] = complement_letter(upper_letter(lo));
        }
        if ((m & 1) && lane == 0) qb[m / 2] = complement_letter(upper_letter(qb[m / 2]));
    }
    if (lane == 0) {
        const int c = turn ? cr : cf, d = turn ? dr : df;
        d0_out[q] = c > 0 ? d : min(max(0, -m), n);
        flag[q] = kToggle ? (uint8_t)(flag[q] ^ (turn ? 1 : 0)) : (uint8_t)(turn ? 1 : 0);
    }
}

// status bit 3 (MP_ANCHOR_REVERSED) of the records whose flag is set: after the last traceback that writes their meta record
__global__ __launch_bounds__(256) void anchor_mark_kernel(int32_t *__restrict__ meta, const uint8_t *__restrict__ flag, int nq) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < nq && flag[q]) meta[(size_t)q * MP_ANCHOR_META + 7] |= MP_ANCHOR_REVERSED;
}

// ---- the banded Gotoh sweep, traced ---------------------------------------------------------------------------------------------------
// Traceback bits of cell (i, t), i = 1 .. m, t = diagonal index inside the band: nibble (i - 1) & 7 of word tb[tb_off[q] + ((i - 1) >> 3) *
// 64 R + t]; bits 0-1: H came from 0 the diagonal, 1 E, 2 F (3: the cell lies outside the matrix); bit 2: E opened here; bit 3: F opened here.
// band_sweep's payload: cell() and outside() form the cell's nibble, add() puts it into acc[r], which collects the nibbles of diagonal
// slot r, eight rows (or the last rows up to m) to a stored word.  Where add() is called is a matter of speed alone (profiles/
// bandsweep.txt): with R >= 4 from joined(), one store site per slot after the two paths have met — half the store sites and a fifth
// fewer branches in the long unrolled step; with R <= 2 behind each of the two calls, where the short step runs 1 .. 3 % faster so.
template <int R>
struct TracePayload {
    static constexpr bool kAddWhereJoined = R >= 4;
    uint32_t *tbq;                             // the query's words
    int m;
    uint32_t acc[R];
    uint32_t bits;                             // the nibble of the cell between its call and joined()
    __device__ __forceinline__ void start(int r, bool) { acc[r] = 0; }
    __device__ __forceinline__ void exchange() {}
    __device__ __forceinline__ void add(int r, int t, int i) {
        const int k = i - 1;
        acc[r] |= bits << (4 * (k & 7));
        if ((k & 7) == 7 || i == m) {
            tbq[(size_t)(k >> 3) * (64 * R) + t] = acc[r];
            acc[r] = 0;
        }
    }
    __device__ __forceinline__ void outside(int r, int t, int i) {
        bits = 3u;
        if (!kAddWhereJoined) add(r, t, i);
    }
    __device__ __forceinline__ void cell(int r, int t, int i, int, bool, int h_source, bool e_opened, bool f_opened, bool) {
        bits = (uint32_t)h_source | (e_opened ? 4u : 0u) | (f_opened ? 8u : 0u);
        if (!kAddWhereJoined) add(r, t, i);
    }
    __device__ __forceinline__ void joined(int r, int t, int i) {
        if (kAddWhereJoined) add(r, t, i);
    }
    __device__ __forceinline__ void finish(int, int) {}
};

// kList (star.hip's band escalation): work item x is record list[x] — d0v and end_out are indexed by the record, tb_off by the item, and the
// item's words start at tb + tb_off[x] - tb_base (a chunk of a longer list).  Without it the item is the record and both are unused.
template <int R, bool kList>
__global__ __launch_bounds__(256) void anchor_dp_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ off, int nq,
                                                         const int32_t *__restrict__ d0v, const uint8_t *__restrict__ acode, int n, int W, int match,
                                                         int mismatch, int open_ext, int ext, int mstride, uint32_t *__restrict__ tb,
                                                         const int64_t *__restrict__ tb_off, int32_t *__restrict__ end_out,
                                                         const int32_t *__restrict__ list, long long tb_base) {
    extern __shared__ uint8_t lds[];           // [npad] anchor codes, then [mstride] query codes per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int npad = (n + 15) & ~15;
    for (int x = threadIdx.x; x < n; x += blockDim.x) lds[x] = acode[x];
    const int item = blockIdx.x * wpb + wave;
    const int q = kList ? (item < nq ? list[item] : 0) : item;
    uint8_t *qc = lds + npad + wave * mstride;
    int m = 0;
    if (item < nq) {
        const uint8_t *qb = bytes + off[q];
        m = (int)(off[q + 1] - off[q]);
        for (int x = lane; x < m; x += 64) qc[x] = (uint8_t)base_code(qb[x]);
    }
    __syncthreads();                           // (the only barrier: what follows is per wave)
    if (item >= nq) return;
    TracePayload<R> pay{tb + (kList ? tb_off[item] - tb_base : tb_off[item]), m};
    const BandEnd end = band_sweep<R>(qc, lds, m, n, d0v[q] - W, W, match, mismatch, open_ext, ext, pay);
    if (lane == 0) {
        end_out[2 * q] = end.score;
        end_out[2 * q + 1] = end.t;
    }
}

// ---- traceback ----------------------------------------------------------------------------------------------------------------------
// kList as in the sweep.  kStore (star.hip's path store): the run of inserted bases met with j anchor positions consumed — a path has at most
// one per j — is noted as run_len[q * slot_stride + j] bases starting at query base q_start[q * slot_stride + j]; entries of other j are
// left as they are.  A run ends where the walk consumes an anchor position (M or D) or reaches row 0, not where the F state was opened:
// with gap_open = 0 the walk leaves and re-enters F at every inserted base of one run.
template <bool kList, bool kStore>
__global__ __launch_bounds__(64) void anchor_trace_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ off, int nq,
                                                           const int32_t *__restrict__ d0v, const uint8_t *__restrict__ acode,
                                                           const int32_t *__restrict__ col, int n, int W, int R, int permille,
                                                           const uint32_t *__restrict__ tb, const int64_t *__restrict__ tb_off,
                                                           const int32_t *__restrict__ end_in, uint8_t *__restrict__ arow, int32_t *__restrict__ meta,
                                                           uint8_t *__restrict__ ops, const int64_t *__restrict__ ops_off,
                                                           const int32_t *__restrict__ list, long long tb_base, uint16_t *__restrict__ run_len,
                                                           uint16_t *__restrict__ q_start, int slot_stride) {
    const int item = blockIdx.x * 64 + threadIdx.x;
    if (item >= nq) return;
    const int q = kList ? list[item] : item;
    const uint8_t *qb = bytes + off[q];
    const int m = (int)(off[q + 1] - off[q]), d0 = d0v[q], dlo = d0 - W, B = 2 * W + 1, Bpad = 64 * R;
    const uint32_t *tbq = tb + (kList ? tb_off[item] - tb_base : tb_off[item]);
    uint8_t *ar = arow + (size_t)q * n;
    int32_t *mt = meta + (size_t)q * MP_ANCHOR_META;
    const int score = end_in[2 * q];
    int t = end_in[2 * q + 1];
    int n_match = 0, n_ins = 0, n_del = 0, j_first = -1, j_last = -1, status = 0;
    if (t < 0) status = 3;
    else {
        uint8_t *op = ops ? ops + ops_off[q + 1] : nullptr;
        int i = m, state = 0, run = 0, run_j = 0;
        bool touch = false;
        // (kStore) the pending run, all of it walked: query bases i .. i + run - 1 in slot run_j
        auto flush = [&]() {
            if (kStore && run) {
                run_len[(size_t)q * slot_stride + run_j] = (uint16_t)run;
                q_start[(size_t)q * slot_stride + run_j] = (uint16_t)i;
                run = 0;
            }
        };
        for (;;) {
            touch = touch || t == 0 || t == B - 1;
            if (state == 0 && i == 0) break;
            const int j = i + dlo + t;
            if (i < 1 || t < 0 || t >= B || j < 0 || j > n) { status |= 4; break; }      // (cannot happen on a path the sweep wrote)
            const uint32_t nib = (tbq[(size_t)((i - 1) >> 3) * Bpad + t] >> (4 * ((i - 1) & 7))) & 15u;
            if (state == 0) {
                const uint32_t src = nib & 3u;
                if (src == 0) {
                    if (j < 1) { status |= 4; break; }
                    flush();
                    const uint8_t ch = qb[i - 1];
                    ar[j - 1] = upper_letter(ch);
                    const int cd = base_code(ch);
                    n_match += cd < 4 && cd == acode[j - 1];
                    if (j_last < 0) j_last = j - 1;
                    j_first = j - 1;
                    if (op) *--op = 'M';
                    i--;
                } else if (src == 3) { status |= 4; break; }
                else state = (int)src;
            } else if (state == 1) {
                if (j < 1) { status |= 4; break; }
                flush();
                ar[j - 1] = '-';
                n_del++;
                if (op) *--op = 'D';
                if (nib & 4u) state = 0;
                t--;
            } else {
                n_ins++;
                if (op) *--op = 'I';
                if (nib & 8u) state = 0;
                i--;
                t++;
                if (kStore) { run++; run_j = j; }
            }
        }
        flush();
        if (touch) status |= 2;
        if ((long long)n_match * 1000 < (long long)permille * m) status |= 1;
    }
    mt[0] = score; mt[1] = d0; mt[2] = n_match; mt[3] = n_ins; mt[4] = n_del;
    mt[5] = j_first >= 0 ? col[j_first] : -1;
    mt[6] = j_last >= 0 ? col[j_last] : -1;
    mt[7] = status; mt[8] = j_first; mt[9] = j_last;
}

}  // namespace

}  // namespace mp
