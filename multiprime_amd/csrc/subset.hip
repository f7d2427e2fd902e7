// subset.hip — part of libmprime_hip.so: the global-optimum degenerate positions of include/mprime_subset.h
// ("V2" = test_data/global_optimum/multiPrime2-core_V2.py, get_Y_position / remove_elements, V2:1236-1291).
//
// Three kernels, shared by the explicit and the resident form:
//   subset_records_kernel   one lane per (search, table entry): the entry's planes XORed with the seed's give the mismatching positions,
//                           gap positions take the seed's base; entries with 1 < |Y| < N + v and at most v gaps are appended to the
//                           search's record segment (mask, count, |Y|) — every step admits a subset of those.
//   subset_sets_kernel      one workgroup per (search, step): OR of the admitted records' masks = T, and how many there are.
//   subset_search_kernel    one workgroup per 1024 ranks of one search (a table of (search, first rank) covers every search of the step,
//                           ragged in |T| and record count).  A lane owns four consecutive ranks: it unranks the first one by the
//                           combinatorial number system, steps to the next three, keeps the four element masks in registers and streams
//                           the records through LDS in tiles of 256; a record adds its count when popcount(mask & ~S) <= v.  The best
//                           (total << 32 | ~rank) of the workgroup goes out with ONE 64-bit atomicMax, the lowest rank whose total equals
//                           cover_number with one atomicMin: neither depends on the order of the workgroups.
// The host side sizes the steps (binomials, the refusals), launches, and — for the rare search whose early exit fired — runs the same
// kernel once more over the ranks below the exit rank (the reference's running maximum at that moment).  No MFMA: bit-mask work.
#include "common.hpp"
#include "../../include/mprime_subset.h"

namespace mp {
namespace {

constexpr int kSubTile = 256;                 // records per LDS tile
constexpr int kSubLaneRanks = 4;              // ranks per lane
constexpr int kSubWgRanks = kBlock * kSubLaneRanks;
constexpr int kSubMaxPick = 128;              // elements a combination can hold (|T| <= 128)
constexpr uint32_t kNoRank = 0xFFFFFFFFu;

struct SubSearch {                            // one search as the kernels see it
    long long ent0;                           // first table entry of its window
    int n_ent;                                // table entries of its window
    long long x0;                             // first extra entry of its window
    int n_x;
    long long rec0;                           // its record segment (n_ent + n_x slots)
    unsigned long long s0, s1;                // the seed's base-index planes
};

__device__ inline unsigned long long ld_word(const void *p, size_t i, int wide) {
    return wide ? static_cast<const unsigned long long *>(p)[i] : (unsigned long long)static_cast<const uint32_t *>(p)[i];
}

__global__ __launch_bounds__(kBlock) void subset_records_kernel(const SubSearch *__restrict__ ss, const long long *__restrict__ work_off, int n_search,
                                                                  const void *b0, const void *b1, const void *g, const uint32_t *__restrict__ count,
                                                                  const void *x_words, int wide, int k, int v, int pc_limit,
                                                                  unsigned long long *__restrict__ rec_lo, unsigned long long *__restrict__ rec_hi,
                                                                  uint32_t *__restrict__ rec_cnt, uint32_t *__restrict__ rec_pc, int *__restrict__ n_rec) {
    const long long total = work_off[n_search];
    const unsigned long long kmask = k >= 64 ? ~0ull : ((1ull << k) - 1);
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        int lo = 0, hi = n_search - 1;                      // the search whose work range holds i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (work_off[mid] <= i) lo = mid; else hi = mid - 1;
        }
        const SubSearch s = ss[lo];
        const int j = (int)(i - work_off[lo]);
        unsigned long long w0, w1, wg;
        uint32_t cn;
        if (j < s.n_ent) {
            const size_t e = (size_t)(s.ent0 + j);
            w0 = ld_word(b0, e, wide); w1 = ld_word(b1, e, wide); wg = ld_word(g, e, wide);
            cn = count[e];
        } else {
            const size_t e = (size_t)(s.x0 + (j - s.n_ent)) * 3;
            w0 = ld_word(x_words, e, wide); w1 = ld_word(x_words, e + 1, wide); wg = ld_word(x_words, e + 2, wide);
            cn = 1;
        }
        const unsigned long long gap = wg & kmask;
        if (__popcll(gap) > v) continue;                   // a gap_sequence key, not a k-mer of `cover`
        const unsigned long long diff = ((w0 ^ s.s0) | (w1 ^ s.s1)) & ~gap & kmask;
        unsigned long long any = diff | gap;
        const int pc = __popcll(any);
        if (pc <= 1 || pc >= pc_limit) continue;
        unsigned long long mlo = 0, mhi = 0;
        while (any) {
            const int p = __ffsll((long long)any) - 1;
            any &= any - 1;
            const bool is_gap = (gap >> p) & 1;
            const unsigned base = is_gap ? (unsigned)(((s.s0 >> p) & 1) | (((s.s1 >> p) & 1) << 1))
                                         : (unsigned)(((w0 >> p) & 1) | (((w1 >> p) & 1) << 1));
            const int id = 4 * p + (int)base;
            if (id < 64) mlo |= 1ull << id; else mhi |= 1ull << (id - 64);
        }
        const int slot = atomicAdd(&n_rec[lo], 1);        // slot < n_ent + n_x: one append per entry at most
        const size_t r = (size_t)(s.rec0 + slot);
        rec_lo[r] = mlo; rec_hi[r] = mhi; rec_cnt[r] = cn; rec_pc[r] = (uint32_t)pc;
    }
}

// grid = n_search * n_steps workgroups; step index st admits |Y| < st + 2 + v
__global__ __launch_bounds__(kBlock) void subset_sets_kernel(const SubSearch *__restrict__ ss, int n_steps, int v, const int *__restrict__ n_rec,
                                                               const unsigned long long *__restrict__ rec_lo, const unsigned long long *__restrict__ rec_hi,
                                                               const uint32_t *__restrict__ rec_pc, unsigned long long *__restrict__ t_mask,
                                                               int *__restrict__ n_adm) {
    __shared__ unsigned long long s_lo[kBlock], s_hi[kBlock];
    __shared__ int s_n[kBlock];
    const int s = (int)(blockIdx.x / (unsigned)n_steps), st = (int)(blockIdx.x % (unsigned)n_steps);
    const uint32_t lim = (uint32_t)(st + 2 + v);
    const long long r0 = ss[s].rec0;
    const int n = n_rec[s];
    unsigned long long lo = 0, hi = 0;
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += kBlock)
        if (rec_pc[r0 + i] < lim) { lo |= rec_lo[r0 + i]; hi |= rec_hi[r0 + i]; cnt++; }
    s_lo[threadIdx.x] = lo; s_hi[threadIdx.x] = hi; s_n[threadIdx.x] = cnt;
    __syncthreads();
    for (int d = kBlock / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            s_lo[threadIdx.x] |= s_lo[threadIdx.x + d]; s_hi[threadIdx.x] |= s_hi[threadIdx.x + d]; s_n[threadIdx.x] += s_n[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        t_mask[2 * (size_t)blockIdx.x] = s_lo[0]; t_mask[2 * (size_t)blockIdx.x + 1] = s_hi[0];
        n_adm[blockIdx.x] = s_n[0];
    }
}

// blocks[b] = (search, first rank); m = dn - 1 elements per combination; binom[n * m + r] = C(n, r) for n <= 128, r < m (saturated; every
// value the unranking compares against a rank below the step's count is exact); limit[s] = ranks of search s in this launch.
__global__ __launch_bounds__(kBlock) void subset_search_kernel(const uint2 *__restrict__ blocks, const SubSearch *__restrict__ ss, int st, int n_steps, int m,
                                                                 int v, const unsigned long long *__restrict__ t_mask, const int *__restrict__ n_rec,
                                                                 const unsigned long long *__restrict__ rec_lo, const unsigned long long *__restrict__ rec_hi,
                                                                 const uint32_t *__restrict__ rec_cnt, const uint32_t *__restrict__ rec_pc,
                                                                 const uint32_t *__restrict__ binom, const uint32_t *__restrict__ limit,
                                                                 const unsigned long long *__restrict__ cover, unsigned long long *__restrict__ best,
                                                                 uint32_t *__restrict__ exit_rank) {
    __shared__ uint8_t s_el[kSubMaxPick];                       // ascending element ids of T
    __shared__ uint8_t s_c[kSubMaxPick][kBlock];                // the lane's combination as indices into s_el, position-major
    __shared__ unsigned long long s_rlo[kSubTile], s_rhi[kSubTile];
    __shared__ uint32_t s_rcnt[kSubTile];
    __shared__ unsigned long long s_best[kBlock];
    __shared__ uint32_t s_exit[kBlock];
    const int tid = threadIdx.x;
    const uint2 blk = blocks[blockIdx.x];
    const int s = (int)blk.x;
    const unsigned long long tlo = t_mask[2 * ((size_t)s * n_steps + st)], thi = t_mask[2 * ((size_t)s * n_steps + st) + 1];
    const int t = __popcll(tlo) + __popcll(thi);
    if (tid < 128) {
        const bool on = tid < 64 ? (tlo >> tid) & 1 : (thi >> (tid - 64)) & 1;
        if (on) {
            const int below = tid < 64 ? __popcll(tlo & ((1ull << tid) - 1)) : __popcll(tlo) + __popcll(thi & ((1ull << (tid - 64)) - 1));
            s_el[below] = (uint8_t)tid;
        }
    }
    __syncthreads();
    const uint32_t lim = limit[s];
    const uint32_t rank0 = blk.y + (uint32_t)tid * kSubLaneRanks;       // blk.y + 1023 < 2^32: the host caps a step at 2^32 - 1 ranks
    const bool mine = blk.y < lim && (uint64_t)blk.y + (uint64_t)tid * kSubLaneRanks < (uint64_t)lim;
    unsigned long long q_lo[kSubLaneRanks], q_hi[kSubLaneRanks];
    if (mine) {
        uint32_t r = rank0;                                              // unrank: lexicographic order of index tuples
        int x = 0;
        for (int i = 0; i < m; i++) {
            while (x < t - 1) {                                          // (x stays inside T whatever the rank)
                const uint32_t c = binom[(size_t)(t - 1 - x) * m + (m - 1 - i)];
                if (r < c) break;
                r -= c;
                x++;
            }
            s_c[i][tid] = (uint8_t)x;
            x++;
        }
    }
#pragma unroll
    for (int q = 0; q < kSubLaneRanks; q++) {
        unsigned long long lo = 0, hi = 0;
        if (mine && (uint64_t)rank0 + q < (uint64_t)lim) {
            if (q) {                                                     // the next combination: raise the last index that can rise
                int i = m - 1;
                while (i >= 0 && (int)s_c[i][tid] == t - m + i) i--;
                if (i >= 0) {
                    int x = s_c[i][tid] + 1;
                    for (; i < m; i++) s_c[i][tid] = (uint8_t)x++;
                }
            }
            for (int i = 0; i < m; i++) {
                const int id = s_el[s_c[i][tid]];
                if (id < 64) lo |= 1ull << id; else hi |= 1ull << (id - 64);
            }
        }
        q_lo[q] = ~lo; q_hi[q] = ~hi;
    }
    uint32_t tot[kSubLaneRanks] = {0, 0, 0, 0};
    const long long r0 = ss[s].rec0;
    const int n = n_rec[s];
    const uint32_t pc_lim = (uint32_t)(m + 1 + v);
    for (int base = 0; base < n; base += kSubTile) {
        __syncthreads();
        const int nt = min(kSubTile, n - base);
        if (tid < nt) {
            const size_t r = (size_t)(r0 + base + tid);
            s_rlo[tid] = rec_lo[r]; s_rhi[tid] = rec_hi[r];
            s_rcnt[tid] = rec_pc[r] < pc_lim ? rec_cnt[r] : 0u;          // not admitted at this step: adds nothing
        }
        __syncthreads();
        for (int j = 0; j < nt; j++) {
            const uint32_t cn = s_rcnt[j];
            if (cn == 0) continue;                                       // (the same for every lane)
            const unsigned long long lo = s_rlo[j], hi = s_rhi[j];
#pragma unroll
            for (int q = 0; q < kSubLaneRanks; q++)
                tot[q] += (__popcll(lo & q_lo[q]) + __popcll(hi & q_hi[q]) <= v) ? cn : 0u;
        }
    }
    unsigned long long b = 0;
    uint32_t ex = kNoRank;
    const unsigned long long cv = cover[s];
#pragma unroll
    for (int q = 0; q < kSubLaneRanks; q++) {
        if (mine && (uint64_t)rank0 + q < (uint64_t)lim) {
            const uint32_t rk = rank0 + q;
            const unsigned long long p = ((unsigned long long)tot[q] << 32) | (unsigned long long)(kNoRank - rk);
            b = p > b ? p : b;
            if ((unsigned long long)tot[q] == cv && rk < ex) ex = rk;
        }
    }
    s_best[tid] = b; s_exit[tid] = ex;
    __syncthreads();
    for (int d = kBlock / 2; d > 0; d >>= 1) {
        if (tid < d) {
            if (s_best[tid + d] > s_best[tid]) s_best[tid] = s_best[tid + d];
            if (s_exit[tid + d] < s_exit[tid]) s_exit[tid] = s_exit[tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (s_best[0]) atomicMax(&best[s], s_best[0]);
        if (s_exit[0] != kNoRank) atomicMin(&exit_rank[s], s_exit[0]);
    }
}

// C(n, r) for n <= 128, r <= 128, saturated at 2^32
struct Binomials {
    uint64_t c[129][129];
    Binomials() {
        const uint64_t sat = 1ull << 32;
        for (int n = 0; n <= 128; n++)
            for (int r = 0; r <= 128; r++)
                c[n][r] = r > n ? 0 : (r == 0 || r == n) ? 1 : std::min(sat, c[n - 1][r - 1] + c[n - 1][r]);
    }
};
const Binomials &binomials() { static const Binomials b; return b; }

inline int popc128(const uint64_t *t) { return __builtin_popcountll(t[0]) + __builtin_popcountll(t[1]); }

struct Tables {                               // the entries both forms search: device arrays + per-window segments on the host
    const void *b0, *b1, *g;
    const uint32_t *count;
    int wide;
    std::vector<int64_t> base;                // [W] first entry of window w
    std::vector<int32_t> n;                   // [W]
};

int run_search(mp_ctx *c, const Tables &tb, int k, int v, int N, int64_t n_extra, const int32_t *x_window, const void *x_words, int n_search,
               const int32_t *s_window, const uint8_t *s_seed, const int64_t *s_cover, uint64_t *t_mask, int32_t *n_admitted,
               int64_t *best_total, int64_t *best_rank, int64_t *exit_rank, int64_t *pre_total) {
    const int W = (int)tb.n.size();
    const int n_steps = N - 1;
    c->sub_ms[0] = c->sub_ms[1] = c->sub_ms[2] = 0;
    if (n_search <= 0 || n_steps <= 0) return MP_OK;
    if (n_steps > kSubMaxPick - 1) return fail(c, MP_ERR_ARG, "multiPrime2: -n %d: at most %d degenerate positions", N, kSubMaxPick);
    if (!s_window || !s_seed || !s_cover || !t_mask || !n_admitted || !best_total || !best_rank || !exit_rank || !pre_total)
        return fail(c, MP_ERR_ARG, "multiPrime2: null argument");
    if (n_extra < 0 || (n_extra && (!x_window || !x_words))) return fail(c, MP_ERR_ARG, "multiPrime2: bad extra entries");
    const size_t wb = tb.wide ? 8 : 4;
    // extra entries grouped by window (stable counting sort on the host: they are few)
    std::vector<int64_t> x_off((size_t)W + 1, 0);
    for (int64_t i = 0; i < n_extra; i++) {
        if (x_window[i] < 0 || x_window[i] >= W) return fail(c, MP_ERR_ARG, "multiPrime2: extra entry %lld names window %d of %d", (long long)i, x_window[i], W);
        x_off[(size_t)x_window[i] + 1]++;
    }
    for (int w = 0; w < W; w++) x_off[(size_t)w + 1] += x_off[(size_t)w];
    std::vector<uint8_t> xw((size_t)std::max<int64_t>(n_extra, 1) * 3 * wb);
    {
        std::vector<int64_t> cur(x_off.begin(), x_off.end() - 1);
        for (int64_t i = 0; i < n_extra; i++)
            memcpy(xw.data() + (size_t)cur[(size_t)x_window[i]]++ * 3 * wb, static_cast<const uint8_t *>(x_words) + (size_t)i * 3 * wb, 3 * wb);
    }
    std::vector<SubSearch> ss((size_t)n_search);
    std::vector<long long> work_off((size_t)n_search + 1, 0);
    std::vector<unsigned long long> cover((size_t)n_search);
    for (int s = 0; s < n_search; s++) {
        const int w = s_window[s];
        if (w < 0 || w >= W) return fail(c, MP_ERR_ARG, "multiPrime2: search %d names window %d of %d", s, w, W);
        SubSearch &x = ss[(size_t)s];
        x.ent0 = tb.base[(size_t)w]; x.n_ent = tb.n[(size_t)w];
        x.x0 = x_off[(size_t)w]; x.n_x = (int)(x_off[(size_t)w + 1] - x_off[(size_t)w]);
        x.rec0 = work_off[(size_t)s];
        x.s0 = x.s1 = 0;
        for (int j = 0; j < k; j++) {
            const uint8_t b = s_seed[(size_t)s * k + j];
            if (b > 3) return fail(c, MP_ERR_ARG, "multiPrime2: seed %d holds base index %d at position %d", s, (int)b, j);
            x.s0 |= (unsigned long long)(b & 1) << j; x.s1 |= (unsigned long long)(b >> 1) << j;
        }
        work_off[(size_t)s + 1] = work_off[(size_t)s] + x.n_ent + x.n_x;
        cover[(size_t)s] = s_cover[s] < 0 ? ~0ull : (unsigned long long)s_cover[s];      // (a total is below 2^32: a larger cover_number never matches)
    }
    const long long n_work = work_off[(size_t)n_search];
    const size_t n_out = (size_t)n_search * (size_t)n_steps;
    for (size_t i = 0; i < n_out; i++) {
        t_mask[2 * i] = t_mask[2 * i + 1] = 0; n_admitted[i] = 0; best_total[i] = 0; best_rank[i] = -1; exit_rank[i] = -1; pre_total[i] = 0;
    }
    HIPCK(c, hipSetDevice(c->dev));
    DevBuf<SubSearch> d_ss(c);
    DevBuf<long long> d_work(c);
    DevBuf<uint8_t> d_xw(c);
    DevBuf<unsigned long long> d_lo(c), d_hi(c), d_t(c), d_cover(c), d_best(c);
    DevBuf<uint32_t> d_cnt(c), d_pc(c), d_binom(c), d_limit(c), d_exit(c);
    DevBuf<int> d_nrec(c), d_nadm(c);
    DevBuf<uint2> d_blocks(c);
    int rc;
    const size_t nrec_cap = (size_t)std::max<long long>(n_work, 1);
    if ((rc = d_ss.alloc(ss.size())) || (rc = d_work.alloc(work_off.size())) || (rc = d_xw.alloc(xw.size())) || (rc = d_lo.alloc(nrec_cap)) ||
        (rc = d_hi.alloc(nrec_cap)) || (rc = d_cnt.alloc(nrec_cap)) || (rc = d_pc.alloc(nrec_cap)) || (rc = d_nrec.alloc((size_t)n_search)) ||
        (rc = d_t.alloc(2 * n_out)) || (rc = d_nadm.alloc(n_out)) || (rc = d_cover.alloc((size_t)n_search)) || (rc = d_best.alloc((size_t)n_search)) ||
        (rc = d_exit.alloc((size_t)n_search)) || (rc = d_limit.alloc((size_t)n_search)))
        return rc;
    HIPCK_WAIT(c, d_ss.upload(ss.data(), ss.size()));
    HIPCK_WAIT(c, d_work.upload(work_off.data(), work_off.size()));
    HIPCK_WAIT(c, d_xw.upload(xw.data(), xw.size()));
    HIPCK_WAIT(c, d_cover.upload(cover.data(), cover.size()));
    HIPCK_WAIT(c, d_nrec.zero());
    StageClock clk[3];
    clk[0].begin(c);
    if (n_work)
        hipLaunchKernelGGL(subset_records_kernel, dim3(std::min(grid(n_work, kBlock), 8192u)), dim3(kBlock), 0, c->stream, d_ss.p, d_work.p, n_search,
                           tb.b0, tb.b1, tb.g, tb.count, (const void *)d_xw.p, tb.wide, k, v, N + v, d_lo.p, d_hi.p, d_cnt.p, d_pc.p, d_nrec.p);
    clk[0].end(c);
    clk[1].begin(c);
    hipLaunchKernelGGL(subset_sets_kernel, dim3((unsigned)n_out), dim3(kBlock), 0, c->stream, d_ss.p, n_steps, v, d_nrec.p, d_lo.p, d_hi.p, d_pc.p,
                       d_t.p, d_nadm.p);
    clk[1].end(c);
    HIPCK_WAIT(c, hipGetLastError());
    HIPCK_WAIT(c, hipMemcpyAsync(t_mask, d_t.p, 16 * n_out, hipMemcpyDeviceToHost, c->stream));
    HIPCK_WAIT(c, hipMemcpyAsync(n_admitted, d_nadm.p, 4 * n_out, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    clk[0].read(&c->sub_ms[0]);
    clk[1].read(&c->sub_ms[1]);
    // the steps: every combination count first (a refusal leaves nothing half done)
    const Binomials &B = binomials();
    for (int s = 0; s < n_search; s++)
        for (int st = 0; st < n_steps; st++) {
            const int t = popc128(t_mask + 2 * ((size_t)s * n_steps + st)), dn = st + 2;
            if (t >= dn && B.c[t][dn - 1] > 0xFFFFFFFFull)
                return fail(c, MP_ERR_ARG, "multiPrime2: search %d (window %d) has C(%d, %d) combinations at step %d: more than 32 bits hold", s,
                            s_window[s], t, dn - 1, dn);
        }
    std::vector<uint2> blocks;
    std::vector<uint32_t> limit((size_t)n_search), binom;
    std::vector<unsigned long long> h_best((size_t)n_search);
    std::vector<uint32_t> h_exit((size_t)n_search);
    auto launch = [&](int st, int m) -> int {          // blocks / limit are set: one launch over every listed search
        if (int rc_a = d_blocks.alloc(blocks.size())) return rc_a;
        HIPCK_WAIT(c, d_blocks.upload(blocks.data(), blocks.size()));
        HIPCK_WAIT(c, d_limit.upload(limit.data(), limit.size()));
        HIPCK_WAIT(c, d_best.zero());
        HIPCK_WAIT(c, hipMemsetAsync(d_exit.p, 0xFF, 4 * (size_t)n_search, c->stream));
        StageClock k3;
        k3.begin(c);
        hipLaunchKernelGGL(subset_search_kernel, dim3((unsigned)blocks.size()), dim3(kBlock), 0, c->stream, d_blocks.p, d_ss.p, st, n_steps, m, v, d_t.p,
                           d_nrec.p, d_lo.p, d_hi.p, d_cnt.p, d_pc.p, d_binom.p, d_limit.p, d_cover.p, d_best.p, d_exit.p);
        k3.end(c);
        HIPCK_WAIT(c, hipGetLastError());
        HIPCK_WAIT(c, hipMemcpyAsync(h_best.data(), d_best.p, 8 * (size_t)n_search, hipMemcpyDeviceToHost, c->stream));
        HIPCK_WAIT(c, hipMemcpyAsync(h_exit.data(), d_exit.p, 4 * (size_t)n_search, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        k3.read(&c->sub_ms[2]);
        return MP_OK;
    };
    auto list_blocks = [&]() {
        blocks.clear();
        for (int s = 0; s < n_search; s++)
            for (uint64_t r = 0; r < limit[(size_t)s]; r += kSubWgRanks) blocks.push_back(make_uint2((unsigned)s, (unsigned)r));
    };
    for (int st = 0; st < n_steps; st++) {
        const int dn = st + 2, m = dn - 1;
        bool any = false;
        for (int s = 0; s < n_search; s++) {
            const int t = popc128(t_mask + 2 * ((size_t)s * n_steps + st));
            limit[(size_t)s] = t >= dn ? (uint32_t)B.c[t][m] : 0u;      // |T| < dn: nothing is launched for this search
            any |= limit[(size_t)s] != 0;
        }
        if (!any) continue;
        binom.assign((size_t)129 * m, 0);
        for (int n = 0; n <= 128; n++)
            for (int r = 0; r < m; r++) binom[(size_t)n * m + r] = (uint32_t)std::min<uint64_t>(B.c[n][r], 0xFFFFFFFFull);
        if ((rc = d_binom.alloc(binom.size()))) return rc;
        HIPCK_WAIT(c, d_binom.upload(binom.data(), binom.size()));
        list_blocks();
        if ((rc = launch(st, m))) return rc;
        bool exits = false;
        for (int s = 0; s < n_search; s++) {
            const size_t o = (size_t)s * n_steps + st;
            const uint32_t lim = limit[(size_t)s];
            limit[(size_t)s] = 0;
            if (!lim) continue;
            best_total[o] = (int64_t)(h_best[(size_t)s] >> 32);
            best_rank[o] = (int64_t)(kNoRank - (uint32_t)(h_best[(size_t)s] & 0xFFFFFFFFull));
            if (h_exit[(size_t)s] != kNoRank) {
                exit_rank[o] = (int64_t)h_exit[(size_t)s];
                limit[(size_t)s] = h_exit[(size_t)s];                     // the ranks below it, once more
                exits |= h_exit[(size_t)s] != 0;
            }
        }
        if (exits) {
            list_blocks();
            if ((rc = launch(st, m))) return rc;
            for (int s = 0; s < n_search; s++)
                if (limit[(size_t)s]) pre_total[(size_t)s * n_steps + st] = (int64_t)(h_best[(size_t)s] >> 32);
        }
    }
    return MP_OK;
}

}  // namespace
}  // namespace mp

using namespace mp;

extern "C" {

int mp_subset_search(mp_ctx *c, int32_t k, int32_t v, int32_t N, int32_t n_windows, const int64_t *win_off, const void *words, const int64_t *counts,
                     int32_t n_search, const int32_t *s_window, const uint8_t *s_seed, const int64_t *s_cover, uint64_t *t_mask, int32_t *n_admitted,
                     int64_t *best_total, int64_t *best_rank, int64_t *exit_rank, int64_t *pre_total) {
    if (!c) return MP_ERR_ARG;
    if (k > MP_SUBSET_MAX_K) return fail(c, MP_ERR_ARG, "multiPrime2: primer length %d: at most %d (an element set is a 128-bit mask)", k, MP_SUBSET_MAX_K);
    if (k < 1 || v < 0 || n_windows < 0 || !win_off) return fail(c, MP_ERR_ARG, "multiPrime2: bad k, v or windows");
    Tables tb;
    tb.wide = k > MP_NARROW_K;
    const int64_t n = win_off[n_windows];
    if (n < 0 || (n && (!words || !counts))) return fail(c, MP_ERR_ARG, "multiPrime2: bad entries");
    std::vector<uint32_t> cnt32((size_t)std::max<int64_t>(n, 1));
    for (int w = 0; w < n_windows; w++) {
        if (win_off[w] > win_off[w + 1] || win_off[w] < 0) return fail(c, MP_ERR_ARG, "multiPrime2: window offsets must ascend");
        uint64_t sum = 0;
        for (int64_t i = win_off[w]; i < win_off[w + 1]; i++) {
            if (counts[i] < 0) return fail(c, MP_ERR_ARG, "multiPrime2: negative count");
            sum += (uint64_t)counts[i];
            if (sum > 0xFFFFFFFFull)
                return fail(c, MP_ERR_ARG, "multiPrime2: the counts of window %d exceed 32 bits (a total and a rank share one 64-bit word)", w);
            cnt32[(size_t)i] = (uint32_t)counts[i];
        }
        tb.base.push_back(win_off[w]);
        tb.n.push_back((int32_t)(win_off[w + 1] - win_off[w]));
    }
    HIPCK(c, hipSetDevice(c->dev));
    const size_t wb = tb.wide ? 8 : 4;
    DevBuf<uint8_t> d_words(c);
    DevBuf<uint32_t> d_cnt(c);
    int rc;
    if ((rc = d_words.alloc(3 * wb * (size_t)std::max<int64_t>(n, 1))) || (rc = d_cnt.alloc(cnt32.size()))) return rc;
    if (n) HIPCK_WAIT(c, d_words.upload(static_cast<const uint8_t *>(words), 3 * wb * (size_t)n));
    HIPCK_WAIT(c, d_cnt.upload(cnt32.data(), cnt32.size()));
    tb.b0 = d_words.p; tb.b1 = d_words.p + wb * (size_t)n; tb.g = d_words.p + 2 * wb * (size_t)n;
    tb.count = d_cnt.p;
    rc = run_search(c, tb, k, v, N, 0, nullptr, nullptr, n_search, s_window, s_seed, s_cover, t_mask, n_admitted, best_total, best_rank, exit_rank,
                    pre_total);
    (void)hipStreamSynchronize(c->stream);      // the uploads above read host arrays of this frame
    return rc;
}

int mp_subset_search_resident(mp_ctx *c, int32_t N, int64_t n_extra, const int32_t *x_window, const void *x_words, int32_t n_search,
                              const int32_t *s_window, const uint8_t *s_seed, const int64_t *s_cover, uint64_t *t_mask, int32_t *n_admitted,
                              int64_t *best_total, int64_t *best_rank, int64_t *exit_rank, int64_t *pre_total) {
    if (!c) return MP_ERR_ARG;
    if (c->h_wbase.empty() || !c->u_b0) return fail(c, MP_ERR_ARG, "multiPrime2: mp_window_unique has not run");
    if (c->k > MP_SUBSET_MAX_K) return fail(c, MP_ERR_ARG, "multiPrime2: primer length %d: at most %d (an element set is a 128-bit mask)", c->k, MP_SUBSET_MAX_K);
    if ((long long)c->n_rows + n_extra > 0xFFFFFFFFll) return fail(c, MP_ERR_ARG, "multiPrime2: the counts of a window may exceed 32 bits");
    Tables tb;
    tb.wide = c->wide;
    tb.b0 = c->u_b0; tb.b1 = c->u_b1; tb.g = c->u_g;
    tb.count = reinterpret_cast<const uint32_t *>(c->u_count);
    tb.base.assign(c->h_wbase.begin(), c->h_wbase.end());
    tb.n.assign(c->h_wcount.begin(), c->h_wcount.end());
    const int rc = run_search(c, tb, c->k, c->v, N, n_extra, x_window, x_words, n_search, s_window, s_seed, s_cover, t_mask, n_admitted, best_total,
                              best_rank, exit_rank, pre_total);
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

int mp_subset_timing(mp_ctx *c, double *ms3) {
    if (!c || !ms3) return MP_ERR_ARG;
    for (int i = 0; i < 3; i++) ms3[i] = c->sub_ms[i];
    return MP_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host replay (no device)
// ---------------------------------------------------------------------------------------------------------------------------------
static bool combination_of_rank(const uint64_t *t, int m, uint64_t rank, uint64_t *out) {
    int el[128], n = 0;
    for (int i = 0; i < 128; i++)
        if ((t[i >> 6] >> (i & 63)) & 1) el[n++] = i;
    const Binomials &B = binomials();
    if (m > n || rank >= B.c[n][m]) return false;
    out[0] = out[1] = 0;
    int x = 0;
    for (int i = 0; i < m; i++) {
        for (;;) {
            const uint64_t cnt = B.c[n - 1 - x][m - 1 - i];
            if (rank < cnt) break;
            rank -= cnt;
            x++;
        }
        out[el[x] >> 6] |= 1ull << (el[x] & 63);
        x++;
    }
    return true;
}

int mp_subset_replay(int32_t k, int32_t N, int32_t n_search, const uint8_t *s_seed, const int64_t *s_cover, const uint64_t *t_mask,
                     const int64_t *best_total, const int64_t *best_rank, const int64_t *exit_rank, const int64_t *pre_total, uint64_t *subset,
                     int64_t *max_count, uint8_t *codes) {
    if (k < 1 || k > MP_SUBSET_MAX_K || n_search < 0 || !s_seed || !s_cover || !subset || !max_count || !codes) return MP_ERR_ARG;
    const int n_steps = N > 1 ? N - 1 : 0;
    if (n_steps && (!t_mask || !best_total || !best_rank || !exit_rank || !pre_total)) return MP_ERR_ARG;
    for (int s = 0; s < n_search; s++) {
        int64_t mc = 0;
        uint64_t sub[2] = {0, 0};
        for (int st = 0; st < n_steps; st++) {
            const size_t o = (size_t)s * n_steps + st;
            const uint64_t *t = t_mask + 2 * o;
            const int dn = st + 2;
            if (popc128(t) >= dn) {
                if (exit_rank[o] >= 0) {                               // V2:1282-1283: the search ends here
                    if (pre_total[o] > mc) mc = pre_total[o];
                    if (!combination_of_rank(t, dn - 1, (uint64_t)exit_rank[o], sub)) return MP_ERR_ARG;
                    break;
                }
                if (best_total[o] > mc) {                              // V2:1284-1286
                    mc = best_total[o];
                    if (best_rank[o] < 0 || !combination_of_rank(t, dn - 1, (uint64_t)best_rank[o], sub)) return MP_ERR_ARG;
                }
            } else {                                                   // V2:1287-1289
                mc = s_cover[s];
                sub[0] = t[0]; sub[1] = t[1];
            }
        }
        subset[2 * (size_t)s] = sub[0]; subset[2 * (size_t)s + 1] = sub[1];
        max_count[s] = mc;
        for (int j = 0; j < k; j++) {
            if (s_seed[(size_t)s * k + j] > 3) return MP_ERR_ARG;
            const int e0 = 4 * j;
            const unsigned add = (unsigned)((sub[e0 >> 6] >> (e0 & 63)) & 15u);       // bit b = base b joins position j (degenerate_merge)
            codes[(size_t)s * k + j] = (uint8_t)((1u << s_seed[(size_t)s * k + j]) | add);
        }
    }
    return MP_OK;
}

int mp_subset_choose(int32_t n_pairs, const int32_t *nm, const int32_t *mm, const int64_t *max_count, int32_t *chosen) {
    if (n_pairs < 0 || !nm || !mm || !max_count || !chosen) return MP_ERR_ARG;
    for (int p = 0; p < n_pairs; p++) chosen[p] = mm[p] < 0 || max_count[nm[p]] >= max_count[mm[p]] ? nm[p] : mm[p];      // V2:1204
    return MP_OK;
}

}  // extern "C"
