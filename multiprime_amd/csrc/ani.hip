// ani.hip — merging rare clusters by identity (include/mprime_ani.h): bottom-s MinHash sketches and their all-pairs comparison reduced
// per pair of groups.  Kernels:
//   ani_sketch_kernel<LOG>  one workgroup per sequence: a lane walks a run of word positions with a rolling 24-bit word and writes the
//                           hashes (0xFFFFFFFF for "no word") into 2^LOG LDS keys; a bitonic sort; then the first s distinct keys go
//                           out behind a ballot-and-prefix compaction, 64 keys per wave and round, until s are written
//   ani_group_kernel        one workgroup per (pair of groups, tile of 8 query sketches, chunk of 64 ref sketches): the tile sits in
//                           LDS, a wave holds one ref sketch in registers (entry i in lane i % 64) and compares it with every sketch of
//                           the tile; per wave (n_rep, sum_ppm) in registers, per workgroup one 64-bit atomic add per output
//   ani_pair_kernel         one wave per pair on the same pair routine, its first sketch in the wave's LDS slice
// Both strands (mp_ani_sketch_strands): ani_sketch_kernel<LOG, true> hashes the smaller of a word and its reverse complement, keeps the
// compacted sketch in LDS and walks the positions once more for the orientation bits; ani_pair_strand_kernel and
// ani_group_strand_kernel are the pair and group kernels' layouts with the bit words beside the sketches, counting (same, opp).
// The work list of a group call is implicit: the host uploads the prefix sums of the workgroups per group pair and a workgroup finds
// its pair by bisection.
#include "common.hpp"
#include "seedword.hpp"
#include "../../include/mprime_ani.h"

#include <cmath>

namespace mp {

namespace {

constexpr int kWord = MP_ANI_WORD;
constexpr uint32_t kNone = 0xFFFFFFFFu;        // no word hashes to it (mprime_ani.h)
constexpr int kMaxS = MP_ANI_MAX_SKETCH;
constexpr int kRegs = kMaxS / 64;              // entries of a sketch per lane
constexpr int kTileQ = 8;                      // query sketches of a workgroup: 32 KiB of LDS at s = 1024
constexpr int kChunkR = 64;                    // ref sketches of a workgroup, 16 per wave

__host__ __device__ inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// ---- sketches ----------------------------------------------------------------------------------------------------------------------------
// list[blockIdx.x]: a sequence with at most 2^LOG word positions.  sk is filled with kNone before the launch.  STRANDS: the canonical
// form — the key is the hash of min(word, reverse-complement word), and orient[seq][(s + 31) / 32] gets the orientation bits.
template <int LOG, bool STRANDS>
__global__ __launch_bounds__(((1 << LOG) / 2 < 1024) ? (1 << LOG) / 2 : 1024) void ani_sketch_kernel(
    const uint8_t *__restrict__ bytes, const int64_t *__restrict__ off, const int32_t *__restrict__ list, int s, uint32_t *__restrict__ sk,
    int32_t *__restrict__ sizes, uint32_t *__restrict__ orient) {
    constexpr int N = 1 << LOG, T = (N / 2 < 1024) ? N / 2 : 1024, CH = N / T, NW = T / 64;
    __shared__ uint32_t keys[N];
    __shared__ int wsum[2][NW];
    __shared__ uint32_t csk[STRANDS ? kMaxS : 1];              // the compacted sketch (4 KiB beside the 128 KiB of the largest sort)
    __shared__ uint32_t seen[STRANDS ? kMaxS / 32 : 1];        // bit i: entry i has an as-read occurrence
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, seq = list[blockIdx.x];
    const int64_t base = off[seq];
    const int len = (int)(off[seq + 1] - base), nw = len - kWord + 1;      // word positions 0 .. nw - 1 (nw <= N; may be <= 0)
    const uint8_t *b = bytes + base;
    {
        const int p0 = t * CH;
        uint32_t w = 0, rcw = 0;               // rcw: the reverse complement of w, its first letter (the last one read, complemented) on top
        int run = 0;                           // valid letters in a row up to the last one read
        if (p0 < nw)
            for (int x = 0; x < kWord - 1; x++) {
                const int cd = base_code(b[p0 + x]);
                run = cd < 4 ? run + 1 : 0;
                w = ((w << 2) | (uint32_t)(cd & 3)) & 0xFFFFFFu;
                if constexpr (STRANDS) rcw = (rcw >> 2) | ((uint32_t)(3 - (cd & 3)) << 22);
            }
        for (int k = 0; k < CH; k++) {
            const int p = p0 + k;
            uint32_t key = kNone;
            if (p < nw) {
                const int cd = base_code(b[p + kWord - 1]);
                run = cd < 4 ? run + 1 : 0;
                w = ((w << 2) | (uint32_t)(cd & 3)) & 0xFFFFFFu;
                if constexpr (STRANDS) rcw = (rcw >> 2) | ((uint32_t)(3 - (cd & 3)) << 22);
                if (run >= kWord) key = fmix32(STRANDS ? min(w, rcw) : w);
            }
            keys[p] = key;
        }
    }
    if constexpr (STRANDS)
        if (t < kMaxS / 32) seen[t] = 0;
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = t; x < N / 2; x += T) {
                const int i = 2 * x - (x & (j - 1)), l = i + j;            // i has bit j clear
                const uint32_t a = keys[i], c = keys[l];
                if ((a > c) == ((i & k) == 0)) { keys[i] = c; keys[l] = a; }
            }
            __syncthreads();
        }
    int have = 0;                              // distinct keys before this round (the same in every lane)
    for (int r0 = 0, round = 0; r0 < N && have < s && keys[r0] != kNone; r0 += T, round++) {       // (sorted: nothing but kNone from there on)
        const int i = r0 + t;
        const uint32_t v = keys[i];
        const bool first = v != kNone && (i == 0 || keys[i - 1] != v);
        const unsigned long long bal = __ballot(first);
        if (lane == 0) wsum[round & 1][wave] = (int)__popcll(bal);
        __syncthreads();                       // (the buffer of round + 2 is written after every wave has passed the barrier of round + 1)
        int before = 0, total = 0;
        for (int x = 0; x < NW; x++) {
            const int n = wsum[round & 1][x];
            total += n;
            if (x < wave) before += n;
        }
        const int pos = have + before + (int)__popcll(bal & ((1ull << lane) - 1ull));
        if (first && pos < s) {
            sk[(size_t)seq * s + pos] = v;
            if constexpr (STRANDS) csk[pos] = v;
        }
        have += total;
    }
    const int size = have < s ? have : s;
    if (t == 0) sizes[seq] = size;
    if constexpr (STRANDS) {
        // The orientation bits: every as-read occurrence (word <= its reverse complement) of a sketched hash sets that entry's bit in
        // `seen`; the stored bit is the complement.  The walk is the one above.
        __syncthreads();
        const uint32_t last = size ? csk[size - 1] : 0;
        const int p0 = t * CH;
        uint32_t w = 0, rcw = 0;
        int run = 0;
        if (p0 < nw && size)
            for (int x = 0; x < kWord - 1; x++) {
                const int cd = base_code(b[p0 + x]);
                run = cd < 4 ? run + 1 : 0;
                w = ((w << 2) | (uint32_t)(cd & 3)) & 0xFFFFFFu;
                rcw = (rcw >> 2) | ((uint32_t)(3 - (cd & 3)) << 22);
            }
        for (int k = 0; k < CH && size; k++) {
            const int p = p0 + k;
            if (p >= nw) break;
            const int cd = base_code(b[p + kWord - 1]);
            run = cd < 4 ? run + 1 : 0;
            w = ((w << 2) | (uint32_t)(cd & 3)) & 0xFFFFFFu;
            rcw = (rcw >> 2) | ((uint32_t)(3 - (cd & 3)) << 22);
            if (run < kWord || w > rcw) continue;
            const uint32_t h = fmix32(w);
            if (h > last) continue;
            int a = 0, n = size;               // the first entry >= h
            while (n > 0) {
                const int half = n >> 1;
                const bool lt = csk[a + half] < h;
                a = lt ? a + half + 1 : a;
                n = lt ? n - half - 1 : half;
            }
            if (a < size && csk[a] == h) atomicOr(&seen[a >> 5], 1u << (a & 31));
        }
        __syncthreads();
        const int nwords = (s + 31) >> 5;
        if (t < nwords) {
            const int left = size - t * 32;    // entries of the sketch from bit 0 of this word on
            const uint32_t mask = left >= 32 ? 0xFFFFFFFFu : left > 0 ? (1u << left) - 1u : 0u;
            orient[(size_t)seq * nwords + t] = ~seen[t] & mask;
        }
    }
}

// ---- a pair -------------------------------------------------------------------------------------------------------------------------------
// Q[0 .. nq): one sketch in LDS; rv[k]: entry k * 64 + lane of the other (kNone past its size nr), rlast its last entry.  Returns w and
// u in every lane.
__device__ inline void pair_counts(const uint32_t *Q, int nq, const uint32_t (&rv)[kRegs], int kr, int nr, uint32_t rlast, int s, int *w_out,
                                   int *u_out) {
    uint32_t c = kNone;                        // no limit: every real entry is below it
    if (nq == s) c = Q[nq - 1];
    if (nr == s) c = min(c, rlast);
    int lo = 0, hi = nq;                       // cq = |{x in Q, x <= c}| (the same search in every lane)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (Q[mid] <= c) lo = mid + 1; else hi = mid;
    }
    const int cq = lo;
    int acc = 0;                               // |{x in R, x <= c}| + (w << 16) of this lane
#pragma unroll
    for (int k = 0; k < kRegs; k++) {
        if (k >= kr) break;
        const uint32_t v = rv[k];
        if (v == kNone || v > c) continue;
        int a = 0, n = cq;
        while (n > 0) {
            const int half = n >> 1;
            const bool lt = Q[a + half] < v;
            a = lt ? a + half + 1 : a;
            n = lt ? n - half - 1 : half;
        }
        acc += 1 + ((a < cq && Q[a] == v) ? (1 << 16) : 0);
    }
    for (int sh = 32; sh >= 1; sh >>= 1) acc += __shfl_xor(acc, sh);
    const int cr = acc & 0xFFFF, w = acc >> 16;
    *w_out = w;
    *u_out = cq + cr - w;
}

__device__ inline void load_regs(const uint32_t *__restrict__ sk, int s, int kr, int lane, uint32_t (&rv)[kRegs]) {
#pragma unroll
    for (int k = 0; k < kRegs; k++) {
        const int i = k * 64 + lane;
        rv[k] = (k < kr && i < s) ? sk[i] : kNone;
    }
}

// item_off[g] .. item_off[g + 1): the workgroups of group pair g, query tiles fastest.  out[g] = {n_rep, sum_ppm}, zeroed before.
__global__ __launch_bounds__(256) void ani_group_kernel(const uint32_t *__restrict__ sk, const int32_t *__restrict__ sizes, int s,
                                                         const int32_t *__restrict__ goff, const int32_t *__restrict__ qg,
                                                         const int32_t *__restrict__ rg, const long long *__restrict__ item_off, long long item0,
                                                         long long n_gp, const uint32_t *__restrict__ tab, uint32_t report,
                                                         unsigned long long *__restrict__ out) {
    __shared__ uint32_t Q[kTileQ * kMaxS];
    __shared__ int qn[kTileQ];
    __shared__ unsigned int red[4][2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long item = item0 + blockIdx.x;
    long long lo = 0, hi = n_gp - 1;           // the last g with item_off[g] <= item (item < item_off[n_gp])
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (item_off[mid] <= item) lo = mid; else hi = mid - 1;
    }
    const long long g = lo;
    const long long local = item - item_off[g];
    const int q0 = goff[qg[g]], nqg = goff[qg[g] + 1] - q0, r0 = goff[rg[g]], nrg = goff[rg[g] + 1] - r0;
    const int nqt = (nqg + kTileQ - 1) / kTileQ;
    const int qa = q0 + (int)(local % nqt) * kTileQ, qcount = min(kTileQ, q0 + nqg - qa);
    const int ra = r0 + (int)(local / nqt) * kChunkR, rcount = min(kChunkR, r0 + nrg - ra);
    for (int x = t; x < qcount * s; x += 256) Q[x] = sk[(size_t)qa * s + x];
    if (t < qcount) qn[t] = sizes[qa + t];
    __syncthreads();
    const int kr = (s + 63) >> 6;
    unsigned int n_rep = 0, sum = 0;           // of this wave: at most 16 * 8 pairs, 1.28e8 ppm
    for (int r = wave; r < rcount; r += 4) {
        const int idx = ra + r, nr = sizes[idx];
        const uint32_t *rs = sk + (size_t)idx * s;
        uint32_t rv[kRegs];
        load_regs(rs, s, kr, lane, rv);
        const uint32_t rlast = nr ? rs[nr - 1] : 0;
        for (int j = 0; j < qcount; j++) {
            int w, u;
            pair_counts(Q + j * s, qn[j], rv, kr, nr, rlast, s, &w, &u);
            const uint32_t ani = tab[u ? (w * 1024) / u : 0];
            if (ani >= report) { n_rep++; sum += ani; }
        }
    }
    if (lane == 0) { red[wave][0] = n_rep; red[wave][1] = sum; }
    __syncthreads();
    if (t == 0) {
        unsigned long long a = 0, b = 0;
        for (int x = 0; x < 4; x++) { a += red[x][0]; b += red[x][1]; }
        if (a) {
            atomicAdd(&out[2 * g], a);
            atomicAdd(&out[2 * g + 1], b);
        }
    }
}

__global__ __launch_bounds__(256) void ani_pair_kernel(const uint32_t *__restrict__ sk, const int32_t *__restrict__ sizes, int s,
                                                        const int32_t *__restrict__ a_idx, const int32_t *__restrict__ b_idx, long long np,
                                                        const uint32_t *__restrict__ tab, int32_t *__restrict__ out) {
    __shared__ uint32_t Q[4 * kMaxS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long p = (long long)blockIdx.x * 4 + wave;
    uint32_t *q = Q + wave * kMaxS;
    if (p < np) {
        const uint32_t *as = sk + (size_t)a_idx[p] * s;
        for (int x = lane; x < s; x += 64) q[x] = as[x];
    }
    __syncthreads();
    if (p >= np) return;
    const int b = b_idx[p], nr = sizes[b], kr = (s + 63) >> 6;
    const uint32_t *rs = sk + (size_t)b * s;
    uint32_t rv[kRegs];
    load_regs(rs, s, kr, lane, rv);
    int w, u;
    pair_counts(q, sizes[a_idx[p]], rv, kr, nr, nr ? rs[nr - 1] : 0, s, &w, &u);
    if (lane == 0) {
        out[3 * p] = w;
        out[3 * p + 1] = u;
        out[3 * p + 2] = (int32_t)tab[u ? (w * 1024) / u : 0];
    }
}

// ---- both strands: (same, opp) of a pair ------------------------------------------------------------------------------------------------
// pair_counts with the orientation bits: QB are the bit words of Q; bit k of rbits is the orientation bit of entry k * 64 + lane of the
// other sketch.  Returns w, u and same (shared entries <= c with equal bits) in every lane.
__device__ inline void pair_counts_strand(const uint32_t *Q, const uint32_t *QB, int nq, const uint32_t (&rv)[kRegs], uint32_t rbits, int kr, int nr,
                                          uint32_t rlast, int s, int *w_out, int *u_out, int *same_out) {
    uint32_t c = kNone;
    if (nq == s) c = Q[nq - 1];
    if (nr == s) c = min(c, rlast);
    int lo = 0, hi = nq;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (Q[mid] <= c) lo = mid + 1; else hi = mid;
    }
    const int cq = lo;
    int acc = 0, same = 0;                     // acc as in pair_counts
#pragma unroll
    for (int k = 0; k < kRegs; k++) {
        if (k >= kr) break;
        const uint32_t v = rv[k];
        if (v == kNone || v > c) continue;
        int a = 0, n = cq;
        while (n > 0) {
            const int half = n >> 1;
            const bool lt = Q[a + half] < v;
            a = lt ? a + half + 1 : a;
            n = lt ? n - half - 1 : half;
        }
        const bool hit = a < cq && Q[a] == v;
        acc += 1 + (hit ? (1 << 16) : 0);
        if (hit && ((QB[a >> 5] >> (a & 31)) & 1u) == ((rbits >> k) & 1u)) same++;
    }
    for (int sh = 32; sh >= 1; sh >>= 1) {
        acc += __shfl_xor(acc, sh);
        same += __shfl_xor(same, sh);
    }
    const int cr = acc & 0xFFFF, w = acc >> 16;
    *w_out = w;
    *u_out = cq + cr - w;
    *same_out = same;
}

// bit k: the orientation bit of entry k * 64 + lane of the sketch whose bit words are ob[0 .. nwords)
__device__ inline uint32_t load_bits(const uint32_t *__restrict__ ob, int nwords, int kr, int lane) {
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < kRegs; k++) {
        const int word = 2 * k + (lane >> 5);
        if (k < kr && word < nwords) out |= ((ob[word] >> (lane & 31)) & 1u) << k;
    }
    return out;
}

// ani_pair_kernel's layout; out[p] = {same, opp}
__global__ __launch_bounds__(256) void ani_pair_strand_kernel(const uint32_t *__restrict__ sk, const int32_t *__restrict__ sizes,
                                                               const uint32_t *__restrict__ orient, int s, const int32_t *__restrict__ a_idx,
                                                               const int32_t *__restrict__ b_idx, long long np, int32_t *__restrict__ out) {
    __shared__ uint32_t Q[4 * kMaxS];
    __shared__ uint32_t QB[4 * (kMaxS / 32)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwords = (s + 31) >> 5;
    const long long p = (long long)blockIdx.x * 4 + wave;
    uint32_t *q = Q + wave * kMaxS, *qb = QB + wave * (kMaxS / 32);
    if (p < np) {
        const uint32_t *as = sk + (size_t)a_idx[p] * s;
        for (int x = lane; x < s; x += 64) q[x] = as[x];
        if (lane < nwords) qb[lane] = orient[(size_t)a_idx[p] * nwords + lane];
    }
    __syncthreads();
    if (p >= np) return;
    const int b = b_idx[p], nr = sizes[b], kr = (s + 63) >> 6;
    const uint32_t *rs = sk + (size_t)b * s;
    uint32_t rv[kRegs];
    load_regs(rs, s, kr, lane, rv);
    const uint32_t rbits = load_bits(orient + (size_t)b * nwords, nwords, kr, lane);
    int w, u, same;
    pair_counts_strand(q, qb, sizes[a_idx[p]], rv, rbits, kr, nr, nr ? rs[nr - 1] : 0, s, &w, &u, &same);
    if (lane == 0) {
        out[2 * p] = same;
        out[2 * p + 1] = w - same;
    }
}

// ani_group_kernel's work list and layout; out[g] = {SAME, OPP} over the reported pairs, zeroed before
__global__ __launch_bounds__(256) void ani_group_strand_kernel(const uint32_t *__restrict__ sk, const int32_t *__restrict__ sizes,
                                                                const uint32_t *__restrict__ orient, int s, const int32_t *__restrict__ goff,
                                                                const int32_t *__restrict__ qg, const int32_t *__restrict__ rg,
                                                                const long long *__restrict__ item_off, long long item0, long long n_gp,
                                                                const uint32_t *__restrict__ tab, uint32_t report, unsigned long long *__restrict__ out) {
    __shared__ uint32_t Q[kTileQ * kMaxS];
    __shared__ uint32_t QB[kTileQ * (kMaxS / 32)];
    __shared__ int qn[kTileQ];
    __shared__ unsigned int red[4][2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwords = (s + 31) >> 5;
    const long long item = item0 + blockIdx.x;
    long long lo = 0, hi = n_gp - 1;           // the last g with item_off[g] <= item (item < item_off[n_gp])
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (item_off[mid] <= item) lo = mid; else hi = mid - 1;
    }
    const long long g = lo;
    const long long local = item - item_off[g];
    const int q0 = goff[qg[g]], nqg = goff[qg[g] + 1] - q0, r0 = goff[rg[g]], nrg = goff[rg[g] + 1] - r0;
    const int nqt = (nqg + kTileQ - 1) / kTileQ;
    const int qa = q0 + (int)(local % nqt) * kTileQ, qcount = min(kTileQ, q0 + nqg - qa);
    const int ra = r0 + (int)(local / nqt) * kChunkR, rcount = min(kChunkR, r0 + nrg - ra);
    for (int x = t; x < qcount * s; x += 256) Q[x] = sk[(size_t)qa * s + x];
    for (int x = t; x < qcount * nwords; x += 256) QB[(x / nwords) * (kMaxS / 32) + x % nwords] = orient[(size_t)qa * nwords + x];
    if (t < qcount) qn[t] = sizes[qa + t];
    __syncthreads();
    const int kr = (s + 63) >> 6;
    unsigned int n_same = 0, n_opp = 0;        // of this wave: at most 16 * 8 pairs of at most 1024 shared entries
    for (int r = wave; r < rcount; r += 4) {
        const int idx = ra + r, nr = sizes[idx];
        const uint32_t *rs = sk + (size_t)idx * s;
        uint32_t rv[kRegs];
        load_regs(rs, s, kr, lane, rv);
        const uint32_t rbits = load_bits(orient + (size_t)idx * nwords, nwords, kr, lane);
        const uint32_t rlast = nr ? rs[nr - 1] : 0;
        for (int j = 0; j < qcount; j++) {
            int w, u, same;
            pair_counts_strand(Q + j * s, QB + j * (kMaxS / 32), qn[j], rv, rbits, kr, nr, rlast, s, &w, &u, &same);
            if (tab[u ? (w * 1024) / u : 0] >= report) { n_same += same; n_opp += w - same; }
        }
    }
    if (lane == 0) { red[wave][0] = n_same; red[wave][1] = n_opp; }
    __syncthreads();
    if (t == 0) {
        unsigned long long a = 0, b = 0;
        for (int x = 0; x < 4; x++) { a += red[x][0]; b += red[x][1]; }
        if (a) atomicAdd(&out[2 * g], a);
        if (b) atomicAdd(&out[2 * g + 1], b);
    }
}

void fill_table(int32_t *tab) {
    tab[0] = 0;
    for (int q = 1; q < MP_ANI_TABLE; q++) {
        const double j = q / 1024.0;
        const double v = std::floor(1e6 * (1.0 + std::log(2.0 * j / (1.0 + j)) / 12.0) + 0.5);
        tab[q] = v > 0 ? (int32_t)v : 0;
    }
}

// Workgroups of one launch.  The runtime does not launch gridDim x blockDim >= 2^32 work-items, so a larger piece of work goes out as
// several launches (the kernels take the first item of theirs).  MP_ANI_MAX_GRID=<workgroups> lowers the cap; read per call.
long long max_grid(int threads) {
    long long cap = ((1LL << 32) - 1) / threads;
    if (const char *e = getenv("MP_ANI_MAX_GRID")) { const long long v = atoll(e); if (v > 0 && v < cap) cap = v; }
    return cap;
}

int dev(mp_ctx *c, hipError_t e, const char *who, const char *what) {
    return e == hipSuccess ? MP_OK : fail(c, MP_ERR_DEVICE, "%s: %s: %s", who, what, hipGetErrorString(e));
}

// device time of what `body` puts on the stream, added to *acc
template <typename F>
int timed(mp_ctx *c, const char *who, double *acc, F body) {
    hipEvent_t ev[2] = {nullptr, nullptr};
    int rc = MP_OK;
    float ms = 0;
    if ((rc = dev(c, hipEventCreate(&ev[0]), who, "hipEventCreate")) == MP_OK && (rc = dev(c, hipEventCreate(&ev[1]), who, "hipEventCreate")) == MP_OK &&
        (rc = dev(c, hipEventRecord(ev[0], c->stream), who, "hipEventRecord")) == MP_OK && (rc = body()) == MP_OK &&
        (rc = dev(c, hipEventRecord(ev[1], c->stream), who, "hipEventRecord")) == MP_OK &&
        (rc = dev(c, hipEventSynchronize(ev[1]), who, "hipEventSynchronize")) == MP_OK &&
        (rc = dev(c, hipEventElapsedTime(&ms, ev[0], ev[1]), who, "hipEventElapsedTime")) == MP_OK)
        *acc += ms;
    else
        (void)hipStreamSynchronize(c->stream);
    for (auto &x : ev) if (x) (void)hipEventDestroy(x);
    return rc;
}

template <int LOG, bool STRANDS>
void launch_sketch_form(mp_ctx *c, const uint8_t *bytes, const int64_t *off, const int32_t *list, int count, int s) {
    constexpr int T = ((1 << LOG) / 2 < 1024) ? (1 << LOG) / 2 : 1024;
    const long long cap = max_grid(T);
    for (long long at = 0; at < count; at += cap)
        hipLaunchKernelGGL((ani_sketch_kernel<LOG, STRANDS>), dim3((unsigned)std::min<long long>(cap, count - at)), dim3(T), 0, c->stream, bytes, off,
                           list + at, s, c->ani_sk, c->ani_sizes, c->ani_or);
}

template <int LOG>
void launch_sketch(mp_ctx *c, const uint8_t *bytes, const int64_t *off, const int32_t *list, int count, int s) {
    if (c->ani_strands) launch_sketch_form<LOG, true>(c, bytes, off, list, count, s);
    else launch_sketch_form<LOG, false>(c, bytes, off, list, count, s);
}

size_t or_words(int s) { return (size_t)MP_ANI_OR_WORDS(s); }

// what every strand call asks of the resident set
int need_strands(mp_ctx *c, const char *who) {
    if (c->ani_n == 0) return fail(c, MP_ERR_ARG, "%s: no sketches (mp_ani_sketch_strands first)", who);
    if (!c->ani_strands) return fail(c, MP_ERR_ARG, "%s: the resident sketches are forward ones (mp_ani_sketch); orientation needs mp_ani_sketch_strands", who);
    return MP_OK;
}

}  // namespace

void free_ani(mp_ctx *c) {
    dev_free(c, &c->ani_or, (size_t)c->ani_n * or_words(c->ani_s));
    c->ani_strands = false;
    dev_free(c, &c->ani_sk, (size_t)c->ani_n * (size_t)c->ani_s);
    dev_free(c, &c->ani_sizes, (size_t)c->ani_n);
    dev_free(c, &c->ani_tab, (size_t)MP_ANI_TABLE);
    c->ani_n = c->ani_s = 0;
}

}  // namespace mp

using namespace mp;

// mp_ani_sketch (forward words) and mp_ani_sketch_strands (canonical words and orientation bits)
static int sketch_set(mp_ctx *c, const char *who, int32_t n, const uint8_t *bytes, const int64_t *off, int32_t s, bool strands) {
    if (!c) return MP_ERR_ARG;
    if (n < 1 || !bytes || !off) return fail(c, MP_ERR_ARG, "%s: bad arguments", who);
    if (s < MP_ANI_MIN_SKETCH || s > MP_ANI_MAX_SKETCH) return fail(c, MP_ERR_ARG, "%s: sketch size %d (%d..%d)", who, s, MP_ANI_MIN_SKETCH, MP_ANI_MAX_SKETCH);
    static const int kLogs[5] = {8, 11, 13, 14, 15};
    std::vector<int32_t> lists[5];
    for (int32_t i = 0; i < n; i++) {
        const int64_t m = off[i + 1] - off[i];
        if (m < 0 || m > MP_ANCHOR_MAX_LEN) return fail(c, MP_ERR_ARG, "%s: record %d has %lld bases (0..%d)", who, i, (long long)m, MP_ANCHOR_MAX_LEN);
        const int64_t nw = m - kWord + 1;
        int k = 0;
        while (nw > (1 << kLogs[k])) k++;      // (32756 words at the most: the last size holds them)
        lists[k].push_back(i);
    }
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    free_ani(c);
    c->ani_ms[0] = c->ani_ms[1] = 0;
    c->ani_counts[0] = c->ani_counts[1] = 0;
    const size_t total = (size_t)(off[n] - off[0]);
    std::vector<int64_t> off0((size_t)n + 1);
    for (int32_t i = 0; i <= n; i++) off0[(size_t)i] = off[i] - off[0];
    std::vector<int32_t> list;
    for (auto &l : lists) list.insert(list.end(), l.begin(), l.end());
    int32_t tab[MP_ANI_TABLE];
    fill_table(tab);
    uint8_t *d_bytes = nullptr;
    int64_t *d_off = nullptr;
    int32_t *d_list = nullptr;
    c->ani_n = n;
    c->ani_s = s;
    c->ani_strands = strands;
    int rc = strands ? dev_alloc(c, &c->ani_or, (size_t)n * or_words(s)) : (int)MP_OK;
    if (rc == MP_OK && (rc = dev_alloc(c, &c->ani_sk, (size_t)n * (size_t)s)) == MP_OK && (rc = dev_alloc(c, &c->ani_sizes, (size_t)n)) == MP_OK &&
        (rc = dev_alloc(c, &c->ani_tab, (size_t)MP_ANI_TABLE)) == MP_OK && (rc = dev_alloc(c, &d_bytes, total)) == MP_OK &&
        (rc = dev_alloc(c, &d_off, (size_t)n + 1)) == MP_OK && (rc = dev_alloc(c, &d_list, (size_t)n)) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_bytes, bytes + off[0], total, hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_off, off0.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_list, list.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(c->ani_tab, tab, sizeof tab, hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK)
        rc = timed(c, who, &c->ani_ms[0], [&]() {
            int rc2;
            if ((rc2 = dev(c, hipMemsetAsync(c->ani_sk, 0xFF, sizeof(uint32_t) * (size_t)n * (size_t)s, c->stream), who, "hipMemsetAsync"))) return rc2;
            if (strands && (rc2 = dev(c, hipMemsetAsync(c->ani_or, 0, sizeof(uint32_t) * (size_t)n * or_words(s), c->stream), who, "hipMemsetAsync"))) return rc2;
            size_t at = 0;
            for (int k = 0; k < 5; k++) {
                const int count = (int)lists[k].size();
                if (!count) continue;
                const int32_t *l = d_list + at;
                at += (size_t)count;
                switch (kLogs[k]) {
                    case 8: launch_sketch<8>(c, d_bytes, d_off, l, count, s); break;
                    case 11: launch_sketch<11>(c, d_bytes, d_off, l, count, s); break;
                    case 13: launch_sketch<13>(c, d_bytes, d_off, l, count, s); break;
                    case 14: launch_sketch<14>(c, d_bytes, d_off, l, count, s); break;
                    default: launch_sketch<15>(c, d_bytes, d_off, l, count, s); break;
                }
                if ((rc2 = dev(c, hipGetLastError(), who, "ani_sketch_kernel"))) return rc2;
            }
            return (int)MP_OK;
        });
    dev_free(c, &d_bytes, total);
    dev_free(c, &d_off, (size_t)n + 1);
    dev_free(c, &d_list, (size_t)n);
    if (rc) { free_ani(c); return rc; }
    c->ani_counts[0] = n;
    return MP_OK;
}

extern "C" {

int mp_ani_table(int32_t *out) {
    if (!out) return MP_ERR_ARG;
    fill_table(out);
    return MP_OK;
}

int mp_ani_sketch(mp_ctx *c, int32_t n, const uint8_t *bytes, const int64_t *off, int32_t s) {
    return sketch_set(c, "mp_ani_sketch", n, bytes, off, s, false);
}

int mp_ani_sketch_strands(mp_ctx *c, int32_t n, const uint8_t *bytes, const int64_t *off, int32_t s) {
    return sketch_set(c, "mp_ani_sketch_strands", n, bytes, off, s, true);
}

int mp_ani_orientations(mp_ctx *c, uint32_t *bits) {
    static const char *who = "mp_ani_orientations";
    if (!c) return MP_ERR_ARG;
    if (int rc = need_strands(c, who)) return rc;
    if (!bits) return fail(c, MP_ERR_ARG, "%s: null argument", who);
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipMemcpy(bits, c->ani_or, sizeof(uint32_t) * (size_t)c->ani_n * or_words(c->ani_s), hipMemcpyDeviceToHost));
    return MP_OK;
}

int mp_ani_pairs_strand(mp_ctx *c, int64_t n_pairs, const int32_t *a_idx, const int32_t *b_idx, int32_t *out) {
    static const char *who = "mp_ani_pairs_strand";
    if (!c) return MP_ERR_ARG;
    if (int rc = need_strands(c, who)) return rc;
    if (n_pairs < 0 || (n_pairs && (!a_idx || !b_idx || !out))) return fail(c, MP_ERR_ARG, "%s: bad arguments", who);
    for (int64_t x = 0; x < n_pairs; x++)
        if (a_idx[x] < 0 || a_idx[x] >= c->ani_n || b_idx[x] < 0 || b_idx[x] >= c->ani_n)
            return fail(c, MP_ERR_ARG, "%s: pair %lld names sequence %d / %d of %d", who, (long long)x, a_idx[x], b_idx[x], c->ani_n);
    if (n_pairs == 0) return MP_OK;
    HIPCK(c, hipSetDevice(c->dev));
    const int64_t batch = std::min<long long>(1 << 24, 4 * max_grid(256));       // four pairs per workgroup
    const size_t cap = (size_t)std::min<int64_t>(n_pairs, batch);
    int32_t *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &d_a, cap)) == MP_OK && (rc = dev_alloc(c, &d_b, cap)) == MP_OK && (rc = dev_alloc(c, &d_out, cap * 2)) == MP_OK)
        for (int64_t p0 = 0; p0 < n_pairs && rc == MP_OK; p0 += batch) {
            const int64_t nb = std::min<int64_t>(batch, n_pairs - p0);
            if ((rc = dev(c, hipMemcpyAsync(d_a, a_idx + p0, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, c->stream), who, "copy")) ||
                (rc = dev(c, hipMemcpyAsync(d_b, b_idx + p0, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, c->stream), who, "copy")))
                break;
            hipLaunchKernelGGL(ani_pair_strand_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, c->stream, (const uint32_t *)c->ani_sk,
                               (const int32_t *)c->ani_sizes, (const uint32_t *)c->ani_or, (int)c->ani_s, (const int32_t *)d_a, (const int32_t *)d_b,
                               (long long)nb, d_out);
            if ((rc = dev(c, hipGetLastError(), who, "ani_pair_strand_kernel")) == MP_OK)
                rc = dev(c, hipMemcpyAsync(out + p0 * 2, d_out, sizeof(int32_t) * (size_t)nb * 2, hipMemcpyDeviceToHost, c->stream), who, "copy");
            if (rc == MP_OK) rc = dev(c, hipStreamSynchronize(c->stream), who, "hipStreamSynchronize");
        }
    (void)hipStreamSynchronize(c->stream);
    dev_free(c, &d_a, cap); dev_free(c, &d_b, cap); dev_free(c, &d_out, cap * 2);
    return rc;
}

int mp_ani_groups_strand(mp_ctx *c, int32_t n_groups, const int32_t *group_off, int64_t n_gp, const int32_t *q_group, const int32_t *r_group,
                         int32_t report_ppm, int64_t *out) {
    static const char *who = "mp_ani_groups_strand";
    if (!c) return MP_ERR_ARG;
    if (int rc = need_strands(c, who)) return rc;
    if (n_groups < 1 || !group_off || n_gp < 0 || (n_gp && (!q_group || !r_group || !out))) return fail(c, MP_ERR_ARG, "%s: bad arguments", who);
    if (report_ppm < 0 || report_ppm > MP_ANI_PPM) return fail(c, MP_ERR_ARG, "%s: report_ppm %d (0..%d)", who, report_ppm, MP_ANI_PPM);
    if (group_off[0] < 0 || group_off[n_groups] > c->ani_n) return fail(c, MP_ERR_ARG, "%s: the groups span %d..%d of %d sequences", who, group_off[0], group_off[n_groups], c->ani_n);
    for (int32_t g = 0; g < n_groups; g++)
        if (group_off[g + 1] < group_off[g]) return fail(c, MP_ERR_ARG, "%s: group %d ends before it starts", who, g);
    std::vector<long long> item_off((size_t)n_gp + 1, 0);
    for (int64_t x = 0; x < n_gp; x++) {
        if (q_group[x] < 0 || q_group[x] >= n_groups || r_group[x] < 0 || r_group[x] >= n_groups)
            return fail(c, MP_ERR_ARG, "%s: pair %lld names group %d / %d of %d", who, (long long)x, q_group[x], r_group[x], n_groups);
        const long long nq = group_off[q_group[x] + 1] - group_off[q_group[x]], nr = group_off[r_group[x] + 1] - group_off[r_group[x]];
        item_off[(size_t)x + 1] = item_off[(size_t)x] + ((nq + kTileQ - 1) / kTileQ) * ((nr + kChunkR - 1) / kChunkR);
    }
    for (int64_t x = 0; x < 2 * n_gp; x++) out[x] = 0;
    const long long items = item_off[(size_t)n_gp];
    if (items == 0) return MP_OK;
    HIPCK(c, hipSetDevice(c->dev));
    int32_t *d_goff = nullptr, *d_q = nullptr, *d_r = nullptr;
    long long *d_item = nullptr;
    unsigned long long *d_out = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &d_goff, (size_t)n_groups + 1)) == MP_OK && (rc = dev_alloc(c, &d_q, (size_t)n_gp)) == MP_OK &&
        (rc = dev_alloc(c, &d_r, (size_t)n_gp)) == MP_OK && (rc = dev_alloc(c, &d_item, (size_t)n_gp + 1)) == MP_OK &&
        (rc = dev_alloc(c, &d_out, (size_t)n_gp * 2)) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_goff, group_off, sizeof(int32_t) * ((size_t)n_groups + 1), hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_q, q_group, sizeof(int32_t) * (size_t)n_gp, hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_r, r_group, sizeof(int32_t) * (size_t)n_gp, hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_item, item_off.data(), sizeof(long long) * ((size_t)n_gp + 1), hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK &&
        (rc = dev(c, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * (size_t)n_gp * 2, c->stream), who, "hipMemsetAsync")) == MP_OK) {
        const long long cap = max_grid(256);
        for (long long i0 = 0; i0 < items && rc == MP_OK; i0 += cap) {
            const long long nb = std::min<long long>(cap, items - i0);
            hipLaunchKernelGGL(ani_group_strand_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, (const uint32_t *)c->ani_sk,
                               (const int32_t *)c->ani_sizes, (const uint32_t *)c->ani_or, (int)c->ani_s, (const int32_t *)d_goff, (const int32_t *)d_q,
                               (const int32_t *)d_r, (const long long *)d_item, i0, (long long)n_gp, (const uint32_t *)c->ani_tab, (uint32_t)report_ppm,
                               d_out);
            rc = dev(c, hipGetLastError(), who, "ani_group_strand_kernel");
        }
    }
    if (rc == MP_OK) rc = dev(c, hipStreamSynchronize(c->stream), who, "hipStreamSynchronize");
    if (rc == MP_OK) rc = dev(c, hipMemcpy(out, d_out, sizeof(int64_t) * (size_t)n_gp * 2, hipMemcpyDeviceToHost), who, "copy");
    (void)hipStreamSynchronize(c->stream);
    dev_free(c, &d_goff, (size_t)n_groups + 1); dev_free(c, &d_q, (size_t)n_gp); dev_free(c, &d_r, (size_t)n_gp);
    dev_free(c, &d_item, (size_t)n_gp + 1); dev_free(c, &d_out, (size_t)n_gp * 2);
    return rc;
}

int mp_ani_sketches(mp_ctx *c, uint32_t *hashes, int32_t *sizes) {
    if (!c) return MP_ERR_ARG;
    if (c->ani_n == 0) return fail(c, MP_ERR_ARG, "mp_ani_sketches: no sketches (mp_ani_sketch first)");
    if (!hashes || !sizes) return fail(c, MP_ERR_ARG, "mp_ani_sketches: null argument");
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipMemcpy(hashes, c->ani_sk, sizeof(uint32_t) * (size_t)c->ani_n * (size_t)c->ani_s, hipMemcpyDeviceToHost));
    HIPCK(c, hipMemcpy(sizes, c->ani_sizes, sizeof(int32_t) * (size_t)c->ani_n, hipMemcpyDeviceToHost));
    return MP_OK;
}

int mp_ani_pairs(mp_ctx *c, int64_t n_pairs, const int32_t *a_idx, const int32_t *b_idx, int32_t *out) {
    static const char *who = "mp_ani_pairs";
    if (!c) return MP_ERR_ARG;
    if (c->ani_n == 0) return fail(c, MP_ERR_ARG, "%s: no sketches (mp_ani_sketch first)", who);
    if (n_pairs < 0 || (n_pairs && (!a_idx || !b_idx || !out))) return fail(c, MP_ERR_ARG, "%s: bad arguments", who);
    for (int64_t x = 0; x < n_pairs; x++)
        if (a_idx[x] < 0 || a_idx[x] >= c->ani_n || b_idx[x] < 0 || b_idx[x] >= c->ani_n)
            return fail(c, MP_ERR_ARG, "%s: pair %lld names sequence %d / %d of %d", who, (long long)x, a_idx[x], b_idx[x], c->ani_n);
    if (n_pairs == 0) return MP_OK;
    HIPCK(c, hipSetDevice(c->dev));
    const int64_t batch = std::min<long long>(1 << 24, 4 * max_grid(256));       // four pairs per workgroup
    const size_t cap = (size_t)std::min<int64_t>(n_pairs, batch);
    int32_t *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &d_a, cap)) == MP_OK && (rc = dev_alloc(c, &d_b, cap)) == MP_OK && (rc = dev_alloc(c, &d_out, cap * MP_ANI_PAIR)) == MP_OK)
        for (int64_t p0 = 0; p0 < n_pairs && rc == MP_OK; p0 += batch) {
            const int64_t nb = std::min<int64_t>(batch, n_pairs - p0);
            if ((rc = dev(c, hipMemcpyAsync(d_a, a_idx + p0, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, c->stream), who, "copy")) ||
                (rc = dev(c, hipMemcpyAsync(d_b, b_idx + p0, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, c->stream), who, "copy")))
                break;
            rc = timed(c, who, &c->ani_ms[1], [&]() {
                hipLaunchKernelGGL(ani_pair_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, c->stream, (const uint32_t *)c->ani_sk,
                                   (const int32_t *)c->ani_sizes, (int)c->ani_s, (const int32_t *)d_a, (const int32_t *)d_b, (long long)nb,
                                   (const uint32_t *)c->ani_tab, d_out);
                return dev(c, hipGetLastError(), who, "ani_pair_kernel");
            });
            if (rc == MP_OK)
                rc = dev(c, hipMemcpy(out + p0 * MP_ANI_PAIR, d_out, sizeof(int32_t) * (size_t)nb * MP_ANI_PAIR, hipMemcpyDeviceToHost), who, "copy");
        }
    (void)hipStreamSynchronize(c->stream);
    dev_free(c, &d_a, cap); dev_free(c, &d_b, cap); dev_free(c, &d_out, cap * MP_ANI_PAIR);
    if (rc == MP_OK) c->ani_counts[1] += n_pairs;
    return rc;
}

int mp_ani_groups(mp_ctx *c, int32_t n_groups, const int32_t *group_off, int64_t n_gp, const int32_t *q_group, const int32_t *r_group,
                  int32_t report_ppm, int64_t *out) {
    static const char *who = "mp_ani_groups";
    if (!c) return MP_ERR_ARG;
    if (c->ani_n == 0) return fail(c, MP_ERR_ARG, "%s: no sketches (mp_ani_sketch first)", who);
    if (n_groups < 1 || !group_off || n_gp < 0 || (n_gp && (!q_group || !r_group || !out))) return fail(c, MP_ERR_ARG, "%s: bad arguments", who);
    if (report_ppm < 0 || report_ppm > MP_ANI_PPM) return fail(c, MP_ERR_ARG, "%s: report_ppm %d (0..%d)", who, report_ppm, MP_ANI_PPM);
    if (group_off[0] < 0 || group_off[n_groups] > c->ani_n) return fail(c, MP_ERR_ARG, "%s: the groups span %d..%d of %d sequences", who, group_off[0], group_off[n_groups], c->ani_n);
    for (int32_t g = 0; g < n_groups; g++)
        if (group_off[g + 1] < group_off[g]) return fail(c, MP_ERR_ARG, "%s: group %d ends before it starts", who, g);
    std::vector<long long> item_off((size_t)n_gp + 1, 0);
    int64_t pairs = 0;
    for (int64_t x = 0; x < n_gp; x++) {
        if (q_group[x] < 0 || q_group[x] >= n_groups || r_group[x] < 0 || r_group[x] >= n_groups)
            return fail(c, MP_ERR_ARG, "%s: pair %lld names group %d / %d of %d", who, (long long)x, q_group[x], r_group[x], n_groups);
        const long long nq = group_off[q_group[x] + 1] - group_off[q_group[x]], nr = group_off[r_group[x] + 1] - group_off[r_group[x]];
        item_off[(size_t)x + 1] = item_off[(size_t)x] + ((nq + kTileQ - 1) / kTileQ) * ((nr + kChunkR - 1) / kChunkR);
        pairs += nq * nr;
    }
    for (int64_t x = 0; x < 2 * n_gp; x++) out[x] = 0;
    const long long items = item_off[(size_t)n_gp];
    if (items == 0) return MP_OK;
    HIPCK(c, hipSetDevice(c->dev));
    int32_t *d_goff = nullptr, *d_q = nullptr, *d_r = nullptr;
    long long *d_item = nullptr;
    unsigned long long *d_out = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &d_goff, (size_t)n_groups + 1)) == MP_OK && (rc = dev_alloc(c, &d_q, (size_t)n_gp)) == MP_OK &&
        (rc = dev_alloc(c, &d_r, (size_t)n_gp)) == MP_OK && (rc = dev_alloc(c, &d_item, (size_t)n_gp + 1)) == MP_OK &&
        (rc = dev_alloc(c, &d_out, (size_t)n_gp * 2)) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_goff, group_off, sizeof(int32_t) * ((size_t)n_groups + 1), hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_q, q_group, sizeof(int32_t) * (size_t)n_gp, hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_r, r_group, sizeof(int32_t) * (size_t)n_gp, hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_item, item_off.data(), sizeof(long long) * ((size_t)n_gp + 1), hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK)
        rc = timed(c, who, &c->ani_ms[1], [&]() {
            int rc2;
            if ((rc2 = dev(c, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * (size_t)n_gp * 2, c->stream), who, "hipMemsetAsync"))) return rc2;
            const long long cap = max_grid(256);
            for (long long i0 = 0; i0 < items; i0 += cap) {
                const long long nb = std::min<long long>(cap, items - i0);
                hipLaunchKernelGGL(ani_group_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, (const uint32_t *)c->ani_sk, (const int32_t *)c->ani_sizes,
                                   (int)c->ani_s, (const int32_t *)d_goff, (const int32_t *)d_q, (const int32_t *)d_r, (const long long *)d_item, i0,
                                   (long long)n_gp, (const uint32_t *)c->ani_tab, (uint32_t)report_ppm, d_out);
                if ((rc2 = dev(c, hipGetLastError(), who, "ani_group_kernel"))) return rc2;
            }
            return (int)MP_OK;
        });
    if (rc == MP_OK) rc = dev(c, hipMemcpy(out, d_out, sizeof(int64_t) * (size_t)n_gp * 2, hipMemcpyDeviceToHost), who, "copy");
    (void)hipStreamSynchronize(c->stream);
    dev_free(c, &d_goff, (size_t)n_groups + 1); dev_free(c, &d_q, (size_t)n_gp); dev_free(c, &d_r, (size_t)n_gp);
    dev_free(c, &d_item, (size_t)n_gp + 1); dev_free(c, &d_out, (size_t)n_gp * 2);
    if (rc == MP_OK) c->ani_counts[1] += pairs;
    return rc;
}

int mp_ani_stats(mp_ctx *c, double *ms, int64_t *counts) {
    if (!c) return MP_ERR_ARG;
    for (int i = 0; i < 2; i++) {
        if (ms) ms[i] = c->ani_ms[i];
        if (counts) counts[i] = c->ani_counts[i];
    }
    return MP_OK;
}

}  // extern "C"
