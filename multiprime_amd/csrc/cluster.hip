// cluster.hip — clustering by identity (include/mprime_cluster.h): greedy incremental clustering in rounds over blocks of candidate
// representatives.  Kernels:
//   cluster_index_kernel  one lane per base of the block's members: the 12-mer that starts there (seedword.hpp) goes into one open-addressing table
//                         of block positions (atomicCAS on the slot; every occurrence is kept, so a lookup walks to the first empty
//                         slot and the order of insertion cannot show)
//   cluster_count_kernel  one wavefront per query: the number of (query position, block position) word matches with members it may
//                         join — the upper bound the host sizes the query's vote table and the candidate buffer from
//   cluster_vote_kernel   one wavefront per query: the same lookups, counted per (member, diagonal) in an open-addressing table of
//                         the wave's own (LDS up to 4096 slots, else a region of a global buffer the host handed out); then the best
//                         diagonal per member under the tie rule by one atomicMax on a packed (votes, rank of d) value; then the
//                         members reaching min_votes are written to the candidate list behind ONE reservation per wave on the
//                         list's cursor (no per-entry atomics on shared state: DESIGN 9.-2).  The list's order is arbitrary; the host
//                         takes minima over it
//   cluster_dp_kernel     one wavefront per candidate pair: band_sweep (bandsweep.hpp: the recurrence, its comparison order and the end
//                         cell, R = 1, 2, 4, 8 diagonals per lane) with the CARRIED-COUNT payload instead of a traceback buffer: H, E
//                         and F each carry the n_match (and the "touched the band's edge" flag) of the predecessor the traceback
//                         would choose, so the end cell holds the traced path's numbers.  Both sequences sit in the wave's LDS
//                         slice; the workgroup is 1 .. 4 waves by the pair's lengths
// The greedy driver, the batching and mp_cluster_pairs are host code below.
#include "bandsweep.hpp"
#include "seedword.hpp"
#include "../../include/mprime_cluster.h"

namespace mp {

namespace {

constexpr int kTouch = 1 << 16;                // above every n_match (<= 32767) in a carried count
constexpr int kLdsSlots = 4096;                // vote table slots a wave keeps in LDS (keys + values: 32 KiB)
constexpr int kRankTop = 131071;               // 17 bits: rank of a diagonal = 2 |d| + (d > 0), smaller is better

__global__ __launch_bounds__(256) void cluster_code_kernel(const uint8_t *__restrict__ bytes, size_t total, uint8_t *__restrict__ code) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g < total) code[g] = (uint8_t)base_code(bytes[g]);
}

// Both strands: sequence n + i of the store is rc(i) in codes — reversed, a code below 4 replaced by its complement 3 - code (A, C, G, T
// are 0 .. 3), every other code kept.  One workgroup per sequence; off holds 2 n + 1 offsets.
__global__ __launch_bounds__(256) void cluster_revcomp_kernel(uint8_t *__restrict__ code, const int64_t *__restrict__ off, int n) {
    const int i = blockIdx.x;
    const int64_t src = off[i], dst = off[n + i];
    const int m = (int)(off[i + 1] - src);
    for (int x = threadIdx.x; x < m; x += 256) {
        const uint8_t cd = code[src + m - 1 - x];
        code[dst + x] = cd < 4 ? (uint8_t)(3 - cd) : cd;
    }
}

// ---- the block index -------------------------------------------------------------------------------------------------------------------
// Members lie back to back in position space: member k owns positions mpos[k] .. mpos[k + 1).
__global__ __launch_bounds__(256) void cluster_index_kernel(const uint8_t *__restrict__ code, const int64_t *__restrict__ off,
                                                             const int32_t *__restrict__ mem_seq, const int32_t *__restrict__ mpos, int nm, int P,
                                                             uint32_t *__restrict__ bkmer, uint16_t *__restrict__ bmem, int32_t *__restrict__ table,
                                                             int log2_slots) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    int lo = 0, hi = nm - 1;                   // the member of position p: the last k with mpos[k] <= p
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (mpos[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int j = p - mpos[lo];
    const int64_t base = off[mem_seq[lo]];
    const int n = (int)(off[mem_seq[lo] + 1] - base);
    const uint32_t w = j + kWord <= n ? seed_word_codes(code + base + j) : kEmpty;
    bkmer[p] = w;
    bmem[p] = (uint16_t)lo;
    if (w == kEmpty) return;
    const uint32_t mask = (1u << log2_slots) - 1;
    uint32_t slot = word_hash(w, log2_slots);
    while (atomicCAS(&table[slot], -1, p) != -1) slot = (slot + 1) & mask;      // (slots >= 2 P: an empty slot exists)
}

// ---- seeds -----------------------------------------------------------------------------------------------------------------------------
// A query may only join members below its limit qlim (inside a block: the members before it; otherwise all).
__global__ __launch_bounds__(256) void cluster_count_kernel(const uint8_t *__restrict__ code, const int64_t *__restrict__ off,
                                                             const int32_t *__restrict__ qseq, const int32_t *__restrict__ qlim, int nq,
                                                             const uint32_t *__restrict__ bkmer, const uint16_t *__restrict__ bmem,
                                                             const int32_t *__restrict__ table, int log2_slots, long long *__restrict__ hits) {
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int64_t base = off[qseq[q]];
    const int m = (int)(off[qseq[q] + 1] - base), lim = qlim[q];
    const uint8_t *qc = code + base;
    const uint32_t mask = (1u << log2_slots) - 1;
    long long cnt = 0;
    for (int i = lane; i + kWord <= m; i += 64) {
        const uint32_t w = seed_word_codes(qc + i);
        if (w == kEmpty) continue;
        uint32_t slot = word_hash(w, log2_slots);
        for (int32_t p; (p = table[slot]) >= 0; slot = (slot + 1) & mask) cnt += bkmer[p] == w && (int)bmem[p] < lim;
    }
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)cnt, sh), hi = __shfl_xor((uint32_t)((unsigned long long)cnt >> 32), sh);
        cnt += (long long)(((unsigned long long)hi << 32) | lo);
    }
    if (lane == 0) hits[q] = cnt;
}

// (what another lane's atomic wrote, not a line of this CU's vector cache)
__device__ inline uint32_t table_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the slot of `key` in the wave's table, claimed when the key is new
__device__ inline uint32_t table_slot(uint32_t *keys, uint32_t key, int log2_cap) {
    const uint32_t mask = (1u << log2_cap) - 1;
    uint32_t s = word_hash(key, log2_cap);
    for (;;) {
        const uint32_t old = atomicCAS(&keys[s], kEmpty, key);
        if (old == kEmpty || old == key) return s;
        s = (s + 1) & mask;
    }
}

// Vote keys: member << 16 | (d + 32768), d + 32768 in 1 .. 65535, value: the votes; the best diagonal of a member under key
// member << 16, value: votes << 17 | (kRankTop - rank of d).  A table of 2^log2_cap > 2 * hits slots holds both kinds (distinct
// diagonals <= hits, members <= distinct diagonals).  Candidates: {query (position in the batch), member, d0, votes}.
__global__ __launch_bounds__(64) void cluster_vote_kernel(const uint8_t *__restrict__ code, const int64_t *__restrict__ off,
                                                           const int32_t *__restrict__ qseq, const int32_t *__restrict__ qlim, int q0,
                                                           const int32_t *__restrict__ mpos, const uint32_t *__restrict__ bkmer,
                                                           const uint16_t *__restrict__ bmem, const int32_t *__restrict__ table, int log2_slots,
                                                           const int32_t *__restrict__ qlog2cap, const long long *__restrict__ qgoff,
                                                           uint32_t *__restrict__ ghash, int min_votes, int4 *__restrict__ cand, unsigned cand_cap,
                                                           unsigned *__restrict__ cursor) {
    __shared__ uint32_t lkeys[kLdsSlots], lvals[kLdsSlots];
    const int lane = threadIdx.x, q = q0 + blockIdx.x;
    const int log2_cap = qlog2cap[q];
    if (log2_cap < 0) return;                  // no word of the query occurs in the block
    const int cap = 1 << log2_cap;
    const long long goff = qgoff[q];
    uint32_t *keys = goff < 0 ? lkeys : ghash + goff, *vals = goff < 0 ? lvals : ghash + goff + cap;
    for (int s = lane; s < cap; s += 64) { keys[s] = kEmpty; vals[s] = 0; }
    __threadfence();
    __syncthreads();
    const int64_t base = off[qseq[q]];
    const int m = (int)(off[qseq[q] + 1] - base), lim = qlim[q];
    const uint8_t *qc = code + base;
    const uint32_t mask = (1u << log2_slots) - 1;
    for (int i = lane; i + kWord <= m; i += 64) {
        const uint32_t w = seed_word_codes(qc + i);
        if (w == kEmpty) continue;
        uint32_t slot = word_hash(w, log2_slots);
        for (int32_t p; (p = table[slot]) >= 0; slot = (slot + 1) & mask) {
            if (bkmer[p] != w) continue;
            const int k = bmem[p];
            if (k >= lim) continue;
            const int d = (p - mpos[k]) - i;                   // -32767 .. 32767
            atomicAdd(&vals[table_slot(keys, ((uint32_t)k << 16) | (uint32_t)(d + 32768), log2_cap)], 1u);
        }
    }
    __threadfence();
    __syncthreads();
    for (int s = lane; s < cap; s += 64) {
        const uint32_t key = table_load(&keys[s]);
        if (key == kEmpty || (key & 0xFFFFu) == 0) continue;
        const int d = (int)(key & 0xFFFFu) - 32768;
        const uint32_t rank = d > 0 ? 2u * (uint32_t)d + 1u : 2u * (uint32_t)(-d);
        atomicMax(&vals[table_slot(keys, key & 0xFFFF0000u, log2_cap)], (table_load(&vals[s]) << 17) | ((uint32_t)kRankTop - rank));
    }
    __threadfence();
    __syncthreads();
    unsigned total = 0;
    for (int s0 = 0; s0 < cap; s0 += 64) {
        const int s = s0 + lane;
        bool ok = false;
        if (s < cap) {
            const uint32_t key = table_load(&keys[s]);
            ok = key != kEmpty && (key & 0xFFFFu) == 0 && (int)(table_load(&vals[s]) >> 17) >= min_votes;
        }
        total += (unsigned)__popcll(__ballot(ok));
    }
    if (total == 0) return;
    unsigned first = 0;
    if (lane == 0) first = atomicAdd(&cursor[0], total);       // one reservation per wave
    first = __shfl(first, 0);
    if (first + total > cand_cap) {                            // (the host sizes the list so that this cannot happen; it checks the flag)
        if (lane == 0) atomicOr(&cursor[1], 1u);
        return;
    }
    for (int s0 = 0; s0 < cap; s0 += 64) {
        const int s = s0 + lane;
        bool ok = false;
        uint32_t key = 0, val = 0;
        if (s < cap) {
            key = table_load(&keys[s]);
            val = table_load(&vals[s]);
            ok = key != kEmpty && (key & 0xFFFFu) == 0 && (int)(val >> 17) >= min_votes;
        }
        const unsigned long long b = __ballot(ok);
        if (ok) {
            const uint32_t rank = (uint32_t)kRankTop - (val & (uint32_t)kRankTop);
            const int ad = (int)(rank >> 1);
            cand[first + (unsigned)__popcll(b & ((1ull << lane) - 1ull))] = make_int4(q, (int)(key >> 16), (rank & 1u) ? ad : -ad, (int)(val >> 17));
        }
        first += (unsigned)__popcll(b);
    }
}

// ---- the banded Gotoh sweep with carried counts ------------------------------------------------------------------------------------------
// band_sweep's payload: H, E and F of every diagonal slot carry the n_match of the path that leads there — the predecessor's count
// by the flags the sweep hands over, one more on a diagonal move that pairs two equal letters.  A count also carries kTouch once a cell
// of its path lies on the band's first or last diagonal.  The end cell's count is the traced path's.
template <int R>
struct CountPayload {
    int HM[R], EM[R], FM[R];
    int hml_edge, eml_edge, hmu_edge, fmu_edge;        // the neighbouring lanes' edge slots as of the step before
    int carried = 0;                                   // the end cell's count
    __device__ __forceinline__ void start(int r, bool on_edge) {
        HM[r] = on_edge ? kTouch : 0;
        EM[r] = FM[r] = 0;
    }
    __device__ __forceinline__ void exchange() {
        hml_edge = __shfl_up(HM[R - 1], 1); eml_edge = __shfl_up(EM[R - 1], 1);
        hmu_edge = __shfl_down(HM[0], 1); fmu_edge = __shfl_down(FM[0], 1);
    }
    // An outside cell keeps whatever its slot carries (as lane 0's left and lane 63's upper edge do, which nobody sets).  That rests on
    // bandsweep.hpp's kNeg < kNoPath and on mprime_anchor.h's limits, (m + n) * MP_ANCHOR_MAX_PARAM < 2^28: an outside cell scores kNeg,
    // everything fed by it alone stays below kNoPath, every score fed by row 0 lies above kNoPath, and a predecessor is chosen by the
    // larger score — so a count that passed through an outside cell is never the one of a reported end cell (none: n_match 0, status 3).
    __device__ __forceinline__ void outside(int, int, int) {}
    __device__ __forceinline__ void cell(int r, int, int, int j, bool on_edge, int h_source, bool e_opened, bool f_opened, bool is_match) {
        const int edge = on_edge ? kTouch : 0;
        const int hml = r > 0 ? HM[r > 0 ? r - 1 : 0] : hml_edge, eml = r > 0 ? EM[r > 0 ? r - 1 : 0] : eml_edge;
        const int hmu = r < R - 1 ? HM[r < R - 1 ? r + 1 : 0] : hmu_edge, fmu = r < R - 1 ? FM[r < R - 1 ? r + 1 : 0] : fmu_edge;
        const int em = (e_opened ? hml : eml) | edge, fm = (f_opened ? hmu : fmu) | edge;
        const int dgm = j >= 1 ? (HM[r] + (is_match ? 1 : 0)) | edge : 0;
        HM[r] = h_source == kFromDiag ? dgm : (h_source == kFromE ? em : fm);
        EM[r] = em; FM[r] = fm;
    }
    __device__ __forceinline__ void joined(int, int, int) {}
    __device__ __forceinline__ void finish(int lane, int r) {
        int mine = 0;
#pragma unroll
        for (int x = 0; x < R; x++) if (x == r) mine = HM[x];
        carried = __shfl(mine, lane);
    }
};

// pairs: {query sequence, anchor sequence, d0, -}; out: {score, n_match, status, -}
template <int R>
__global__ __launch_bounds__(256) void cluster_dp_kernel(const uint8_t *__restrict__ code, const int64_t *__restrict__ off,
                                                          const int4 *__restrict__ pairs, int np, int W, int match, int mismatch, int open_ext, int ext,
                                                          int permille, int stride, int4 *__restrict__ out) {
    extern __shared__ uint8_t lds[];           // per wave [stride]: the anchor's codes, then (16-aligned) the query's
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int p = blockIdx.x * wpb + wave;
    uint8_t *ac = lds + (size_t)wave * stride, *qc = ac;
    int m = 0, n = 0, d0 = 0;
    if (p < np) {
        const int4 pr = pairs[p];
        const int64_t qb = off[pr.x], ab = off[pr.y];
        m = (int)(off[pr.x + 1] - qb);
        n = (int)(off[pr.y + 1] - ab);
        d0 = pr.z;
        qc = ac + ((n + 15) & ~15);
        for (int x = lane; x < n; x += 64) ac[x] = code[ab + x];
        for (int x = lane; x < m; x += 64) qc[x] = code[qb + x];
    }
    __syncthreads();                           // (the only barrier: what follows is per wave)
    if (p >= np) return;
    CountPayload<R> pay;
    const BandEnd end = band_sweep<R>(qc, ac, m, n, d0 - W, W, match, mismatch, open_ext, ext, pay);
    if (lane == 0) {
        const bool none = end.t < 0;
        const int n_match = none ? 0 : (pay.carried & (kTouch - 1));
        int status = none ? 3 : ((pay.carried & kTouch) ? 2 : 0);
        if ((long long)n_match * 1000 < (long long)permille * m) status |= 1;
        out[p] = make_int4(end.score, n_match, status, 0);
    }
}

long long env_cap(const char *name, long long dflt) {
    if (const char *s = getenv(name)) { const long long v = atoll(s); if (v > 0) return v; }
    return dflt;
}

struct Cand { int32_t q, member, d0, votes; };      // q: position in the query list of the seeding
struct PairIn { int32_t q, r, d0, pad; };           // sequence numbers
struct PairOut { int32_t score, n_match, status, pad; };

// The device buffers and limits of one call.
struct Run {
    mp_ctx *c;
    mp_cluster_params par;
    hipEvent_t ev[2] = {nullptr, nullptr};
    // the block index
    int32_t max_members = 0, max_pos = 0, nm = 0, log2_slots = 0;
    int32_t *d_mem = nullptr, *d_mpos = nullptr, *d_table = nullptr;
    uint32_t *d_bkmer = nullptr;
    uint16_t *d_bmem = nullptr;
    size_t table_slots = 0;
    // seeds
    int32_t qbatch = 0;
    int32_t *d_qseq = nullptr, *d_qlim = nullptr, *d_qlog2cap = nullptr;
    long long *d_hits = nullptr, *d_qgoff = nullptr;
    uint32_t *d_ghash = nullptr;
    size_t ghash_words = 0;
    int4 *d_cand = nullptr;
    size_t cand_cap = 0;
    unsigned *d_cursor = nullptr;
    // alignment
    long long pbatch = 0;
    int4 *d_pairs = nullptr, *d_out = nullptr;

    explicit Run(mp_ctx *ctx, const mp_cluster_params &p) : c(ctx), par(p) {}
    ~Run() {
        (void)hipStreamSynchronize(c->stream);
        for (auto &x : ev) if (x) (void)hipEventDestroy(x);
        dev_free(c, &d_mem, (size_t)max_members); dev_free(c, &d_mpos, (size_t)max_members + 1); dev_free(c, &d_table, table_slots);
        dev_free(c, &d_bkmer, (size_t)max_pos); dev_free(c, &d_bmem, (size_t)max_pos);
        dev_free(c, &d_qseq, (size_t)qbatch); dev_free(c, &d_qlim, (size_t)qbatch); dev_free(c, &d_qlog2cap, (size_t)qbatch);
        dev_free(c, &d_hits, (size_t)qbatch); dev_free(c, &d_qgoff, (size_t)qbatch); dev_free(c, &d_ghash, ghash_words);
        dev_free(c, &d_cand, cand_cap); dev_free(c, &d_cursor, (size_t)2);
        dev_free(c, &d_pairs, (size_t)pbatch); dev_free(c, &d_out, (size_t)pbatch);
    }
    int dev(hipError_t e, const char *what) { return e == hipSuccess ? MP_OK : fail(c, MP_ERR_DEVICE, "mp_cluster: %s: %s", what, hipGetErrorString(e)); }
    int64_t len(int32_t s) const { return c->cl_off_host[(size_t)s + 1] - c->cl_off_host[(size_t)s]; }

    // Buffers sized from the free device memory: an eighth each for the vote tables and for the block index, 64 MB at the most for the
    // candidate list and the pair batch.
    int setup(int32_t want_members) {
        int rc;
        if ((rc = dev(hipSetDevice(c->dev), "hipSetDevice"))) return rc;
        for (auto &x : ev) if ((rc = dev(hipEventCreate(&x), "hipEventCreate"))) return rc;
        size_t free_b = 0, total_b = 0;
        if ((rc = dev(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo"))) return rc;
        // a position of the index costs 4 (word) + 2 (member) + 2 slots x 4 bytes, rounded up to the power of two: at most 22 bytes
        const size_t pos_budget = std::min<size_t>(std::max<size_t>(free_b / 8 / 22, (size_t)1 << 16), (size_t)1 << 24);
        max_members = (int32_t)std::min<long long>(std::min<long long>(want_members, MP_CLUSTER_MAX_BLOCK), std::max<long long>(c->cl_n, 1));
        // a block always takes its first member, whatever its length
        max_pos = (int32_t)std::max<size_t>(pos_budget, (size_t)MP_ANCHOR_MAX_LEN);
        size_t total = c->cl_total;
        if ((size_t)max_pos > total) max_pos = (int32_t)std::max<size_t>(total, 1);
        table_slots = 16;
        while (table_slots < 2 * (size_t)max_pos) table_slots <<= 1;
        // (the free memory read above is what the store left: with the reverse copies resident the budgets below count the doubled store)
        qbatch = (int32_t)std::min<long long>(std::max<long long>((c->cl_rev ? 2LL : 1LL) * c->cl_n, 1), 1 << 18);
        ghash_words = std::min<size_t>(std::max<size_t>(free_b / 8 / 4, (size_t)1 << 22), (size_t)1 << 28);
        cand_cap = std::max<size_t>((size_t)1 << 22, (size_t)max_members);
        pbatch = env_cap("MP_CLUSTER_PAIR_BATCH", 1 << 22);
        pbatch = std::min<long long>(pbatch, 1 << 22);
        if ((rc = dev_alloc(c, &d_mem, (size_t)max_members)) || (rc = dev_alloc(c, &d_mpos, (size_t)max_members + 1)) ||
            (rc = dev_alloc(c, &d_table, table_slots)) || (rc = dev_alloc(c, &d_bkmer, (size_t)max_pos)) || (rc = dev_alloc(c, &d_bmem, (size_t)max_pos)) ||
            (rc = dev_alloc(c, &d_qseq, (size_t)qbatch)) || (rc = dev_alloc(c, &d_qlim, (size_t)qbatch)) || (rc = dev_alloc(c, &d_qlog2cap, (size_t)qbatch)) ||
            (rc = dev_alloc(c, &d_hits, (size_t)qbatch)) || (rc = dev_alloc(c, &d_qgoff, (size_t)qbatch)) || (rc = dev_alloc(c, &d_ghash, ghash_words)) ||
            (rc = dev_alloc(c, &d_cand, cand_cap)) || (rc = dev_alloc(c, &d_cursor, (size_t)2)) || (rc = dev_alloc(c, &d_pairs, (size_t)pbatch)) ||
            (rc = dev_alloc(c, &d_out, (size_t)pbatch)))
            return rc;
        return MP_OK;
    }

    // device time between tic() and toc(), added to *acc (toc waits for the stream)
    int tic() { return dev(hipEventRecord(ev[0], c->stream), "hipEventRecord"); }
    int toc(double *acc) {
        int rc;
        float ms = 0;
        if ((rc = dev(hipEventRecord(ev[1], c->stream), "hipEventRecord")) || (rc = dev(hipEventSynchronize(ev[1]), "hipEventSynchronize")) ||
            (rc = dev(hipEventElapsedTime(&ms, ev[0], ev[1]), "hipEventElapsedTime")))
            return rc;
        *acc += ms;
        return MP_OK;
    }

    // how many of the sequences seqs[from ..) one block takes: at most max_members, their bases within max_pos (one at least)
    size_t block_size(const std::vector<int32_t> &seqs, size_t from) const {
        size_t k = from;
        int64_t pos = 0;
        while (k < seqs.size() && k - from < (size_t)max_members && (k == from || pos + len(seqs[k]) <= max_pos)) pos += len(seqs[k++]);
        return k - from;
    }

    int index(const std::vector<int32_t> &members) {
        nm = (int32_t)members.size();
        std::vector<int32_t> mpos((size_t)nm + 1, 0);
        for (int32_t k = 0; k < nm; k++) mpos[(size_t)k + 1] = mpos[(size_t)k] + (int32_t)len(members[(size_t)k]);
        const int32_t P = mpos[(size_t)nm];
        log2_slots = 4;
        while (((size_t)1 << log2_slots) < 2 * (size_t)P) log2_slots++;
        int rc;
        if ((rc = dev(hipMemcpyAsync(d_mem, members.data(), sizeof(int32_t) * (size_t)nm, hipMemcpyHostToDevice, c->stream), "copy")) ||
            (rc = dev(hipMemcpyAsync(d_mpos, mpos.data(), sizeof(int32_t) * ((size_t)nm + 1), hipMemcpyHostToDevice, c->stream), "copy")) ||
            (rc = dev(hipStreamSynchronize(c->stream), "sync")) || (rc = tic()) ||
            (rc = dev(hipMemsetAsync(d_table, 0xFF, sizeof(int32_t) << log2_slots, c->stream), "hipMemsetAsync")))
            return rc;
        hipLaunchKernelGGL(cluster_index_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)c->cl_code,
                           (const int64_t *)c->cl_off, (const int32_t *)d_mem, (const int32_t *)d_mpos, (int)nm, (int)P, d_bkmer, d_bmem, d_table, (int)log2_slots);
        if ((rc = dev(hipGetLastError(), "cluster_index_kernel"))) return rc;
        return toc(&c->cl_ms[0]);
    }

    // The candidates of queries[] (sequence numbers; lim[] their member limits) against the indexed block: every (query, member < limit)
    // whose best diagonal has at least max(1, min_votes) votes, in no particular order.
    int seed(const std::vector<int32_t> &queries, const std::vector<int32_t> &lim, int min_votes, std::vector<Cand> *out) {
        std::vector<long long> hits, goff;
        std::vector<int32_t> l2cap;
        std::vector<size_t> cuts;
        int rc;
        for (size_t b0 = 0; b0 < queries.size(); b0 += (size_t)qbatch) {
            const int32_t nb = (int32_t)std::min<size_t>((size_t)qbatch, queries.size() - b0);
            if ((rc = dev(hipMemcpyAsync(d_qseq, queries.data() + b0, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, c->stream), "copy")) ||
                (rc = dev(hipMemcpyAsync(d_qlim, lim.data() + b0, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, c->stream), "copy")) || (rc = tic()))
                return rc;
            hipLaunchKernelGGL(cluster_count_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, c->stream, (const uint8_t *)c->cl_code,
                               (const int64_t *)c->cl_off, (const int32_t *)d_qseq, (const int32_t *)d_qlim, (int)nb, (const uint32_t *)d_bkmer,
                               (const uint16_t *)d_bmem, (const int32_t *)d_table, (int)log2_slots, d_hits);
            if ((rc = dev(hipGetLastError(), "cluster_count_kernel")) || (rc = toc(&c->cl_ms[1]))) return rc;
            hits.resize((size_t)nb);
            if ((rc = dev(hipMemcpy(hits.data(), d_hits, sizeof(long long) * (size_t)nb, hipMemcpyDeviceToHost), "copy"))) return rc;
            // the vote table of every query, and the cuts where a launch's global tables or candidates would outgrow their buffers
            goff.assign((size_t)nb, -1);
            l2cap.assign((size_t)nb, -1);
            cuts.assign(1, 0);
            size_t words = 0, cands = 0;
            for (int32_t q = 0; q < nb; q++) {
                const long long h = hits[(size_t)q];
                if (h == 0) continue;
                int l2 = 1;
                while (l2 < 62 && (1LL << l2) < 2 * h + 1) l2++;
                const size_t region = l2 < 40 ? (size_t)2 << l2 : (size_t)-1;
                if ((1LL << l2) > kLdsSlots && region > ghash_words)
                    return fail(c, MP_ERR_CAPACITY, "mp_cluster: record %d shares %lld 12-mer occurrences with one block of representatives: its vote table exceeds the device budget (a low-complexity record?)",
                                queries[b0 + (size_t)q], h);
                const size_t need_c = (size_t)std::min<long long>(h, lim[b0 + (size_t)q]);
                const size_t need_w = (1LL << l2) > kLdsSlots ? region : 0;
                if (words + need_w > ghash_words || cands + need_c > cand_cap) { cuts.push_back((size_t)q); words = cands = 0; }
                l2cap[(size_t)q] = l2;
                if (need_w) { goff[(size_t)q] = (long long)words; words += need_w; }
                cands += need_c;
            }
            cuts.push_back((size_t)nb);
            if ((rc = dev(hipMemcpyAsync(d_qlog2cap, l2cap.data(), sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, c->stream), "copy")) ||
                (rc = dev(hipMemcpyAsync(d_qgoff, goff.data(), sizeof(long long) * (size_t)nb, hipMemcpyHostToDevice, c->stream), "copy")))
                return rc;
            for (size_t x = 0; x + 1 < cuts.size(); x++) {
                const size_t a = cuts[x], b = cuts[x + 1];
                if (a == b) continue;
                if ((rc = dev(hipMemsetAsync(d_cursor, 0, 2 * sizeof(unsigned), c->stream), "hipMemsetAsync")) || (rc = tic())) return rc;
                hipLaunchKernelGGL(cluster_vote_kernel, dim3((unsigned)(b - a)), dim3(64), 0, c->stream, (const uint8_t *)c->cl_code, (const int64_t *)c->cl_off,
                                   (const int32_t *)d_qseq, (const int32_t *)d_qlim, (int)a, (const int32_t *)d_mpos, (const uint32_t *)d_bkmer,
                                   (const uint16_t *)d_bmem, (const int32_t *)d_table, (int)log2_slots, (const int32_t *)d_qlog2cap, (const long long *)d_qgoff,
                                   d_ghash, std::max(1, min_votes), d_cand, (unsigned)cand_cap, d_cursor);
                if ((rc = dev(hipGetLastError(), "cluster_vote_kernel")) || (rc = toc(&c->cl_ms[1]))) return rc;
                unsigned cur[2] = {0, 0};
                if ((rc = dev(hipMemcpy(cur, d_cursor, sizeof cur, hipMemcpyDeviceToHost), "copy"))) return rc;
                if (cur[1] || cur[0] > cand_cap) return fail(c, MP_ERR_DEVICE, "mp_cluster: the candidate list overflowed (%u of %zu)", cur[0], cand_cap);
                const size_t at = out->size();
                out->resize(at + cur[0]);
                if (cur[0] && (rc = dev(hipMemcpy(out->data() + at, d_cand, sizeof(Cand) * (size_t)cur[0], hipMemcpyDeviceToHost), "copy"))) return rc;
                for (size_t i = at; i < out->size(); i++) (*out)[i].q += (int32_t)b0;
            }
        }
        return MP_OK;
    }

    // every (query, member < limit) the seeding left out, without a vote: what min_votes = 0 aligns as well
    void complete(const std::vector<int32_t> &lim, std::vector<Cand> *cands) const {
        std::sort(cands->begin(), cands->end(), [](const Cand &a, const Cand &b) { return a.q != b.q ? a.q < b.q : a.member < b.member; });
        std::vector<Cand> all;
        size_t x = 0;
        for (int32_t q = 0; q < (int32_t)lim.size(); q++)
            for (int32_t k = 0; k < lim[(size_t)q]; k++) {
                if (x < cands->size() && (*cands)[x].q == q && (*cands)[x].member == k) all.push_back((*cands)[x++]);
                else all.push_back(Cand{q, k, 0, 0});
            }
        cands->swap(all);
    }

    int align(const std::vector<PairIn> &pairs, std::vector<PairOut> *out) {
        out->assign(pairs.size(), PairOut{MP_ANCHOR_NO_SCORE, 0, 3, 0});
        if (pairs.empty()) return MP_OK;
        const int W = par.band, B = 2 * W + 1;
        auto stride_of = [&](const PairIn &p) { return (int)(((len(p.r) + 15) & ~15LL) + ((len(p.q) + 15) & ~15LL)); };
        // long pairs first: a launch takes pairs whose LDS slices differ by less than two, its workgroup as many waves as 32 KiB hold (1 .. 4)
        std::vector<uint32_t> order(pairs.size());
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return stride_of(pairs[a]) > stride_of(pairs[b]); });
        std::vector<PairIn> staged;
        std::vector<PairOut> got;
        int rc;
        for (size_t b0 = 0; b0 < order.size(); b0 += (size_t)pbatch) {
            const size_t nb = std::min<size_t>((size_t)pbatch, order.size() - b0);
            staged.resize(nb);
            for (size_t x = 0; x < nb; x++) staged[x] = pairs[order[b0 + x]];
            if ((rc = dev(hipMemcpyAsync(d_pairs, staged.data(), sizeof(PairIn) * nb, hipMemcpyHostToDevice, c->stream), "copy")) || (rc = tic())) return rc;
            for (size_t a = 0; a < nb;) {
                const int stride = stride_of(staged[a]);
                size_t b = a + 1;
                while (b < nb && 2 * stride_of(staged[b]) > stride) b++;
                const int wpb = std::max(1, std::min(4, 32768 / stride));
                const size_t lds = (size_t)wpb * (size_t)stride;       // at most 64 KiB: one wave, two sequences of 32767 bases
                const int np = (int)(b - a);
                const dim3 grid((unsigned)((np + wpb - 1) / wpb)), block((unsigned)(64 * wpb));
                for_lane_diagonals(W, [&](auto r) {
                    hipLaunchKernelGGL((cluster_dp_kernel<decltype(r)::value>), grid, block, lds, c->stream, (const uint8_t *)c->cl_code,
                                       (const int64_t *)c->cl_off, (const int4 *)(d_pairs + a), np, W, (int)par.match, (int)par.mismatch,
                                       (int)(par.gap_open + par.gap_extend), (int)par.gap_extend, (int)par.identity_permille, stride, d_out + a);
                });
                if ((rc = dev(hipGetLastError(), "cluster_dp_kernel"))) return rc;
                a = b;
            }
            if ((rc = toc(&c->cl_ms[2]))) return rc;
            got.resize(nb);
            if ((rc = dev(hipMemcpy(got.data(), d_out, sizeof(PairOut) * nb, hipMemcpyDeviceToHost), "copy"))) return rc;
            for (size_t x = 0; x < nb; x++) {
                (*out)[order[b0 + x]] = got[x];
                c->cl_counts[2] += len(staged[x].q) * B;
            }
        }
        c->cl_counts[1] += (int64_t)pairs.size();
        return MP_OK;
    }
};

int check_params(mp_ctx *c, const char *who, const mp_cluster_params *p) {
    const int32_t sc[4] = {p->match, p->mismatch, p->gap_open, p->gap_extend};
    for (int i = 0; i < 4; i++)
        if (sc[i] < 0 || sc[i] > MP_ANCHOR_MAX_PARAM) return fail(c, MP_ERR_ARG, "%s: score parameter %d (0..%d)", who, sc[i], MP_ANCHOR_MAX_PARAM);
    if (p->band < 0 || p->band > MP_ANCHOR_MAX_BAND) return fail(c, MP_ERR_ARG, "%s: band %d (0..%d)", who, p->band, MP_ANCHOR_MAX_BAND);
    if (p->identity_permille < 0 || p->identity_permille > 1000) return fail(c, MP_ERR_ARG, "%s: identity_permille %d (0..1000)", who, p->identity_permille);
    if (p->min_votes < 0 || p->min_votes > MP_ANCHOR_MAX_LEN) return fail(c, MP_ERR_ARG, "%s: min_votes %d (0..%d)", who, p->min_votes, MP_ANCHOR_MAX_LEN);
    return MP_OK;
}

void reset_stats(mp_ctx *c) {
    for (double &x : c->cl_ms) x = 0;
    for (int64_t &x : c->cl_counts) x = 0;
}

// The reverse copies, built on the device from the resident codes on the first both-strand call: the store grows to 2 cl_total codes
// and 2 cl_n + 1 offsets; cl_n and cl_total keep counting the forward half.
int ensure_reverse(mp_ctx *c, const char *who) {
    if (c->cl_rev) return MP_OK;
    const size_t n = (size_t)c->cl_n, total = c->cl_total;
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    std::vector<int64_t> off2(2 * n + 1);
    for (size_t i = 0; i <= n; i++) off2[i] = c->cl_off_host[i];
    for (size_t i = 1; i <= n; i++) off2[n + i] = (int64_t)total + c->cl_off_host[i];
    uint8_t *code2 = nullptr;
    int64_t *d_off2 = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &code2, 2 * total)) || (rc = dev_alloc(c, &d_off2, 2 * n + 1))) {
        dev_free(c, &code2, 2 * total);
        dev_free(c, &d_off2, 2 * n + 1);
        return rc;
    }
    hipError_t e = hipMemcpyAsync(code2, c->cl_code, total, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off2, off2.data(), sizeof(int64_t) * (2 * n + 1), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cluster_revcomp_kernel, dim3((unsigned)n), dim3(256), 0, c->stream, code2, (const int64_t *)d_off2, (int)n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        dev_free(c, &code2, 2 * total);
        dev_free(c, &d_off2, 2 * n + 1);
        return fail(c, MP_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    }
    dev_free(c, &c->cl_code, total);
    dev_free(c, &c->cl_off, n + 1);
    c->cl_code = code2;
    c->cl_off = d_off2;
    c->cl_off_host.swap(off2);
    c->cl_rev = true;
    return MP_OK;
}

}  // namespace

void free_cluster(mp_ctx *c) {
    const size_t k = c->cl_rev ? 2 : 1;
    dev_free(c, &c->cl_code, k * c->cl_total);
    dev_free(c, &c->cl_off, k * (size_t)c->cl_n + 1);
    c->cl_rev = false;
    c->cl_n = 0;
    c->cl_total = 0;
    c->cl_off_host.clear();
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_cluster_load(mp_ctx *c, int32_t n, const uint8_t *bytes, const int64_t *off) {
    if (!c) return MP_ERR_ARG;
    if (n < 1 || !bytes || !off) return fail(c, MP_ERR_ARG, "mp_cluster_load: bad arguments");
    for (int32_t i = 0; i < n; i++) {
        const int64_t m = off[i + 1] - off[i];
        if (m < 1 || m > MP_ANCHOR_MAX_LEN) return fail(c, MP_ERR_ARG, "mp_cluster_load: record %d has %lld bases (1..%d)", i, (long long)m, MP_ANCHOR_MAX_LEN);
    }
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    free_cluster(c);
    const size_t total = (size_t)(off[n] - off[0]);
    c->cl_n = n;
    c->cl_total = total;
    c->cl_off_host.resize((size_t)n + 1);
    for (int32_t i = 0; i <= n; i++) c->cl_off_host[(size_t)i] = off[i] - off[0];
    uint8_t *d_bytes = nullptr;
    int rc;
    if ((rc = dev_alloc(c, &c->cl_code, total)) || (rc = dev_alloc(c, &c->cl_off, (size_t)n + 1)) || (rc = dev_alloc(c, &d_bytes, total))) {
        dev_free(c, &d_bytes, total);
        free_cluster(c);
        return rc;
    }
    hipError_t e = hipMemcpyAsync(d_bytes, bytes + off[0], total, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->cl_off, c->cl_off_host.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(cluster_code_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)d_bytes, total, c->cl_code);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(c, &d_bytes, total);
    if (e != hipSuccess) { free_cluster(c); return fail(c, MP_ERR_DEVICE, "mp_cluster_load: %s", hipGetErrorString(e)); }
    return MP_OK;
}

}  // extern "C"

namespace {

// mp_cluster_pairs (q_strand == null) and mp_cluster_pairs_strands: the query of pair x is sequence q_idx[x], or its reverse copy
// cl_n + q_idx[x] of the store where q_strand[x] is set; anchors are forward copies.
int pairs_impl(mp_ctx *c, const char *who, int64_t n_pairs, const int32_t *q_idx, const int32_t *r_idx, const int32_t *q_strand,
               const mp_cluster_params *p, int32_t *out) {
    int rc;
    if ((rc = check_params(c, who, p))) return rc;
    for (int64_t x = 0; x < n_pairs; x++) {
        if (q_idx[x] < 0 || q_idx[x] >= c->cl_n || r_idx[x] < 0 || r_idx[x] >= c->cl_n)
            return fail(c, MP_ERR_ARG, "%s: pair %lld names sequence %d / %d of %d", who, (long long)x, q_idx[x], r_idx[x], c->cl_n);
        if (q_strand && (q_strand[x] < 0 || q_strand[x] > 1)) return fail(c, MP_ERR_ARG, "%s: pair %lld names strand %d (0 or 1)", who, (long long)x, q_strand[x]);
    }
    if (q_strand && n_pairs && (rc = ensure_reverse(c, who))) return rc;
    const int32_t n_seq = c->cl_n;
    auto qseq = [&](int64_t x) { return q_strand && q_strand[x] ? n_seq + q_idx[x] : q_idx[x]; };
    const auto t0 = std::chrono::steady_clock::now();
    reset_stats(c);
    if (n_pairs == 0) return MP_OK;
    Run run(c, *p);
    if ((rc = run.setup((int32_t)env_cap("MP_CLUSTER_BLOCK", 2048)))) return rc;
    // pairs by anchor: the anchors of a run of them are one block, the queries of those pairs are seeded against it
    std::vector<int64_t> order((size_t)n_pairs);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return r_idx[a] < r_idx[b]; });
    std::vector<int32_t> anchors;
    for (int64_t x : order) if (anchors.empty() || anchors.back() != r_idx[x]) anchors.push_back(r_idx[x]);
    std::vector<int32_t> members, queries, lim, q_of((q_strand ? 2 : 1) * (size_t)c->cl_n, -1);
    std::vector<Cand> cands;
    std::vector<PairIn> pin;
    std::vector<PairOut> pout;
    std::vector<int64_t> pin_of;
    size_t at = 0;                             // in `order`
    for (size_t a0 = 0; a0 < anchors.size();) {
        const size_t nb = run.block_size(anchors, a0);
        members.assign(anchors.begin() + (long)a0, anchors.begin() + (long)(a0 + nb));
        a0 += nb;
        size_t end = at;
        queries.clear();
        while (end < order.size() && r_idx[order[end]] <= members.back()) {
            const int32_t q = qseq(order[end++]);
            if (q_of[(size_t)q] < 0) { q_of[(size_t)q] = (int32_t)queries.size(); queries.push_back(q); }
        }
        lim.assign(queries.size(), (int32_t)members.size());
        cands.clear();
        if ((rc = run.index(members)) || (rc = run.seed(queries, lim, 1, &cands))) return rc;
        std::sort(cands.begin(), cands.end(), [](const Cand &a, const Cand &b) { return a.q != b.q ? a.q < b.q : a.member < b.member; });
        pin.clear();
        pin_of.clear();
        for (size_t x = at; x < end; x++) {
            const int64_t pi = order[x];
            const int32_t k = (int32_t)(std::lower_bound(members.begin(), members.end(), r_idx[pi]) - members.begin());
            const Cand key{q_of[(size_t)qseq(pi)], k, 0, 0};
            const auto it = std::lower_bound(cands.begin(), cands.end(), key, [](const Cand &a, const Cand &b) { return a.q != b.q ? a.q < b.q : a.member < b.member; });
            const bool hit = it != cands.end() && it->q == key.q && it->member == k;
            int32_t *o = out + (size_t)pi * MP_CLUSTER_PAIR;
            o[0] = hit ? it->votes : 0;
            o[1] = hit ? it->d0 : 0;
            o[2] = MP_ANCHOR_NO_SCORE; o[3] = 0; o[4] = MP_CLUSTER_NOT_SEEDED | 1;
            if (o[0] >= p->min_votes) { pin.push_back(PairIn{qseq(pi), r_idx[pi], o[1], 0}); pin_of.push_back(pi); }
        }
        if ((rc = run.align(pin, &pout))) return rc;
        for (size_t x = 0; x < pin.size(); x++) {
            int32_t *o = out + (size_t)pin_of[x] * MP_CLUSTER_PAIR;
            o[2] = pout[x].score; o[3] = pout[x].n_match; o[4] = pout[x].status;
        }
        for (int32_t q : queries) q_of[(size_t)q] = -1;
        at = end;
        c->cl_counts[0]++;
    }
    c->cl_ms[4] = ms_since(t0);
    return MP_OK;
}

// mp_cluster_greedy (strand_of == null) and mp_cluster_greedy_strands.  Both strands: a seeding's query list is the forward copies
// followed by their reverse copies cl_n + s, so candidate q >= nq is the reverse copy of query q - nq; similar_pairs aligns the
// forward candidates first and then the reverse candidates of the (query, member) pairs whose forward test did not hold — per
// representative "forward first, then reverse", and a pair yields at most one join, which carries its strand.  Representatives and
// indexed members are forward copies throughout.
int greedy_impl(mp_ctx *c, const char *who, const mp_cluster_params *p, int32_t *cluster_of, int32_t *rep_of_cluster, int32_t *n_match_of,
                int32_t *strand_of, int32_t *n_clusters) {
    int rc;
    if ((rc = check_params(c, who, p))) return rc;
    const bool both = strand_of != nullptr;
    if (both && (rc = ensure_reverse(c, who))) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    reset_stats(c);
    Run run(c, *p);
    if ((rc = run.setup((int32_t)env_cap("MP_CLUSTER_BLOCK", 2048)))) return rc;
    const int32_t n = c->cl_n;
    std::vector<int32_t> rest((size_t)n);      // the unassigned sequences in processing order
    std::iota(rest.begin(), rest.end(), 0);
    std::stable_sort(rest.begin(), rest.end(), [&](int32_t a, int32_t b) { return run.len(a) > run.len(b); });
    for (int32_t i = 0; i < n; i++) cluster_of[i] = -1;
    if (both) for (int32_t i = 0; i < n; i++) strand_of[i] = 0;
    int32_t nc = 0;
    struct Join { int32_t q, member, n_match, strand; };
    std::vector<int32_t> members, reps, queries, lim, best, best_nm, best_strand;
    std::vector<Cand> cands;
    std::vector<PairIn> pin;
    std::vector<PairOut> pout;
    std::vector<Join> joins;
    std::vector<char> real;
    std::vector<Cand> rcands;
    std::vector<uint64_t> held;
    // queries -> (queries, their reverse copies), lim -> (lim, lim)
    auto both_strands = [&]() {
        const size_t nq = queries.size();
        queries.resize(2 * nq);
        lim.resize(2 * nq);
        for (size_t x = 0; x < nq; x++) { queries[nq + x] = n + queries[x]; lim[nq + x] = lim[x]; }
    };
    auto similar_pairs = [&](const std::vector<int32_t> &anchors, const std::vector<int32_t> &qs) {      // cands -> joins
        if (p->min_votes == 0) run.complete(lim, &cands);
        const int32_t nq = both ? (int32_t)(qs.size() / 2) : (int32_t)qs.size();
        if (both) {            // the reverse candidates wait for the forward results
            rcands.clear();
            size_t keep = 0;
            for (const Cand &cd : cands) { if (cd.q >= nq) rcands.push_back(cd); else cands[keep++] = cd; }
            cands.resize(keep);
        }
        pin.resize(cands.size());
        for (size_t x = 0; x < cands.size(); x++) pin[x] = PairIn{qs[(size_t)cands[x].q], anchors[(size_t)cands[x].member], cands[x].d0, 0};
        int rc2 = run.align(pin, &pout);
        joins.clear();
        if (rc2) return rc2;
        for (size_t x = 0; x < cands.size(); x++)
            if (!(pout[x].status & 1)) joins.push_back(Join{cands[x].q, cands[x].member, pout[x].n_match, 0});
        if (!both) return (int)MP_OK;
        held.resize(joins.size());
        for (size_t x = 0; x < joins.size(); x++) held[x] = ((uint64_t)(uint32_t)joins[x].q << 32) | (uint32_t)joins[x].member;
        std::sort(held.begin(), held.end());
        size_t keep = 0;
        for (const Cand &cd : rcands)
            if (!std::binary_search(held.begin(), held.end(), ((uint64_t)(uint32_t)(cd.q - nq) << 32) | (uint32_t)cd.member)) rcands[keep++] = cd;
        rcands.resize(keep);
        pin.resize(rcands.size());
        for (size_t x = 0; x < rcands.size(); x++) pin[x] = PairIn{qs[(size_t)rcands[x].q], anchors[(size_t)rcands[x].member], rcands[x].d0, 0};
        if ((rc2 = run.align(pin, &pout))) return rc2;
        for (size_t x = 0; x < rcands.size(); x++)
            if (!(pout[x].status & 1)) joins.push_back(Join{rcands[x].q - nq, rcands[x].member, pout[x].n_match, 1});
        return (int)MP_OK;
    };
    while (!rest.empty()) {
        const size_t nb = run.block_size(rest, 0);
        members.assign(rest.begin(), rest.begin() + (long)nb);
        // (1) the block against itself: member k may join the members before it
        cands.clear();
        joins.clear();
        if (nb > 1) {
            queries.assign(members.begin() + 1, members.end());
            lim.resize(nb - 1);
            std::iota(lim.begin(), lim.end(), 1);
            if (both) both_strands();
            if ((rc = run.index(members)) || (rc = run.seed(queries, lim, p->min_votes, &cands)) || (rc = similar_pairs(members, queries))) return rc;
        }
        // (2) in order: a member is a representative iff no earlier real representative of the block is similar to it
        auto t1 = std::chrono::steady_clock::now();
        real.assign(nb, 0);
        std::sort(joins.begin(), joins.end(), [](const Join &a, const Join &b) { return a.q != b.q ? a.q < b.q : a.member < b.member; });
        reps.clear();
        size_t jx = 0;
        for (size_t k = 0; k < nb; k++) {
            int32_t to = -1, nm = 0, strand = 0;
            for (; jx < joins.size() && (size_t)joins[jx].q + 1 == k; jx++)
                if (to < 0 && real[(size_t)joins[jx].member]) { to = joins[jx].member; nm = joins[jx].n_match; strand = joins[jx].strand; }
            const int32_t s = members[k];
            if (to < 0) {
                real[k] = 1;
                reps.push_back(s);
                rep_of_cluster[nc] = s;
                cluster_of[s] = nc++;
                n_match_of[s] = (int32_t)run.len(s);
            } else {
                cluster_of[s] = cluster_of[members[(size_t)to]];
                n_match_of[s] = nm;
                if (both) strand_of[s] = strand;
            }
        }
        c->cl_ms[3] += ms_since(t1);
        // (3) every later unassigned sequence against the block's representatives; (4) it joins the smallest-numbered one that passes
        queries.assign(rest.begin() + (long)nb, rest.end());
        if (!queries.empty()) {
            const size_t nq = queries.size();
            lim.assign(nq, (int32_t)reps.size());
            if (both) both_strands();
            cands.clear();
            if ((rc = run.index(reps)) || (rc = run.seed(queries, lim, p->min_votes, &cands)) || (rc = similar_pairs(reps, queries))) return rc;
            t1 = std::chrono::steady_clock::now();
            best.assign(nq, -1);
            best_nm.assign(nq, 0);
            best_strand.assign(nq, 0);
            for (const Join &j : joins)
                if (best[(size_t)j.q] < 0 || j.member < best[(size_t)j.q]) { best[(size_t)j.q] = j.member; best_nm[(size_t)j.q] = j.n_match; best_strand[(size_t)j.q] = j.strand; }
            rest.clear();
            for (size_t x = 0; x < nq; x++) {
                const int32_t s = queries[x];
                if (best[x] < 0) { rest.push_back(s); continue; }
                cluster_of[s] = cluster_of[reps[(size_t)best[x]]];
                n_match_of[s] = best_nm[x];
                if (both) strand_of[s] = best_strand[x];
            }
            c->cl_ms[3] += ms_since(t1);
        } else rest.clear();
        c->cl_counts[0]++;
    }
    *n_clusters = nc;
    c->cl_ms[4] = ms_since(t0);
    return MP_OK;
}

}  // namespace

extern "C" {

int mp_cluster_pairs(mp_ctx *c, int64_t n_pairs, const int32_t *q_idx, const int32_t *r_idx, const mp_cluster_params *p, int32_t *out) {
    if (!c) return MP_ERR_ARG;
    if (c->cl_n == 0) return fail(c, MP_ERR_ARG, "mp_cluster_pairs: no sequences (mp_cluster_load first)");
    if (n_pairs < 0 || !p || (n_pairs && (!q_idx || !r_idx || !out))) return fail(c, MP_ERR_ARG, "mp_cluster_pairs: bad arguments");
    return pairs_impl(c, "mp_cluster_pairs", n_pairs, q_idx, r_idx, nullptr, p, out);
}

int mp_cluster_pairs_strands(mp_ctx *c, int64_t n_pairs, const int32_t *q_idx, const int32_t *r_idx, const int32_t *q_strand, const mp_cluster_params *p,
                             int32_t *out) {
    if (!c) return MP_ERR_ARG;
    if (c->cl_n == 0) return fail(c, MP_ERR_ARG, "mp_cluster_pairs_strands: no sequences (mp_cluster_load first)");
    if (n_pairs < 0 || !p || (n_pairs && (!q_idx || !r_idx || !q_strand || !out))) return fail(c, MP_ERR_ARG, "mp_cluster_pairs_strands: bad arguments");
    return pairs_impl(c, "mp_cluster_pairs_strands", n_pairs, q_idx, r_idx, q_strand, p, out);
}

int mp_cluster_greedy(mp_ctx *c, const mp_cluster_params *p, int32_t *cluster_of, int32_t *rep_of_cluster, int32_t *n_match_of, int32_t *n_clusters) {
    if (!c) return MP_ERR_ARG;
    if (c->cl_n == 0) return fail(c, MP_ERR_ARG, "mp_cluster_greedy: no sequences (mp_cluster_load first)");
    if (!p || !cluster_of || !rep_of_cluster || !n_match_of || !n_clusters) return fail(c, MP_ERR_ARG, "mp_cluster_greedy: null argument");
    return greedy_impl(c, "mp_cluster_greedy", p, cluster_of, rep_of_cluster, n_match_of, nullptr, n_clusters);
}

int mp_cluster_greedy_strands(mp_ctx *c, const mp_cluster_params *p, int32_t *cluster_of, int32_t *rep_of_cluster, int32_t *n_match_of, int32_t *strand_of,
                              int32_t *n_clusters) {
    if (!c) return MP_ERR_ARG;
    if (c->cl_n == 0) return fail(c, MP_ERR_ARG, "mp_cluster_greedy_strands: no sequences (mp_cluster_load first)");
    if (!p || !cluster_of || !rep_of_cluster || !n_match_of || !strand_of || !n_clusters) return fail(c, MP_ERR_ARG, "mp_cluster_greedy_strands: null argument");
    return greedy_impl(c, "mp_cluster_greedy_strands", p, cluster_of, rep_of_cluster, n_match_of, strand_of, n_clusters);
}

int mp_cluster_stats(mp_ctx *c, double *ms, int64_t *counts) {
    if (!c) return MP_ERR_ARG;
    for (int i = 0; i < 5; i++) if (ms) ms[i] = c->cl_ms[i];
    for (int i = 0; i < 3; i++) if (counts) counts[i] = c->cl_counts[i];
    return MP_OK;
}

}  // extern "C"
