// dege.hip — DegePrime's degenerate oligomer per window (include/mprime_dege.h).  Kernels:
//   dege_code_kernel        bytes -> 5-bit codes, stored column by column (a wave's loads of one column coalesce); the first byte outside
//                           the alphabet is found with an integer atomicMin on its index
//   dege_extent_kernel      one lane per row: first and last letter
//   dege_window_lds_kernel  one workgroup of 1024 per window: the distinct mers of the spanning rows counted in an LDS table (a slot is claimed
//                           with the first row's number, a hit is verified against that row's symbols), the gap-free ones sorted by their
//                           2-bit word, the counts of all of them sorted and run-length coded
//   dege_window_glb_kernel  the same routine with the table and the sort arrays in global memory, for the windows the first one gave up
//   dege_prefix_kernel      inclusive prefix sums of a window's sorted counts
//   dege_merge_kernel       one workgroup per printed window, one wavefront per iteration of the rule
// Integers only on the device; the entropy is summed on the host from the (count, multiplicity) pairs.
#include "common.hpp"
#include "../../include/mprime_dege.h"

#include <cmath>

namespace mp {

struct WinRec { int32_t n_span, n_free, n_uniq, n_pairs; long long off; };       // n_uniq = -1: the LDS table gave up

struct DegeState {
    int32_t n_rows = 0, width = 0;
    uint8_t *code = nullptr;                 // [width][n_rows]
    int32_t *start = nullptr, *end = nullptr;
    // windows
    int32_t l = 0, skip = 0, depth = 0, n_win = 0, pair_stride = 0;
    WinRec *win = nullptr;                   // [n_win]
    uint64_t *u_words = nullptr;             // [u_cap] sorted unique mers, window w at win[w].off
    uint32_t *u_cnt = nullptr, *u_pre = nullptr;     // their counts / inclusive prefix sums
    uint32_t *pairs = nullptr;               // [n_win][pair_stride][2] (c, m_c), unordered
    long long u_cap = 0, u_total = 0;
    std::vector<WinRec> h_win;
    std::vector<double> h_entropy;
    // merging
    int32_t max_deg = 0, iters = 0, n_printed = 0;
    uint64_t seed = 0;
    int32_t *best = nullptr;                 // [n_win][MP_DEGE_REC]
    int32_t *list = nullptr;                 // [n_printed] printed windows
    bool merged = false;
    double ms[2] = {0, 0};
    int64_t n_global = 0;
};

namespace {

constexpr int kSlots = MP_DEGE_LDS_SLOTS, kLimit = MP_DEGE_LDS_LIMIT, kSortMin = MP_DEGE_SORT_MIN, kMergeLds = MP_DEGE_MERGE_LDS;
constexpr int kRec = MP_DEGE_REC, kDraws = MP_DEGE_MAX_DRAWS;
constexpr int kWindowThreads = 1024;          // the table and the sort arrays take a few bytes more than 80 KiB of LDS: one workgroup per CU, so it is a full one (sixteen wavefronts hide the latency of the byte loads)
constexpr int kMergeThreads = 1024;           // sixteen wavefronts share a window's mers: an iteration is a chain of dependent steps, so more of them run abreast
constexpr uint8_t kBad = 255, kGap = 15, kDot = 31;
constexpr unsigned long long kNoBad = ~0ull;

__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
    return z;
}

// ---- load ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dege_code_kernel(const uint8_t *__restrict__ raw, const uint8_t *__restrict__ lut, long long total,
                                                         int n_rows, int width, uint8_t *__restrict__ code, unsigned long long *__restrict__ bad) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / width), col = (int)(i % width);
        uint8_t c = lut[raw[i]];
        if (c == kBad) { atomicMin(bad, (unsigned long long)i); c = kGap; }
        code[(size_t)col * (size_t)n_rows + (size_t)r] = c;
    }
}

__global__ __launch_bounds__(256) void dege_extent_kernel(const uint8_t *__restrict__ code, int n_rows, int width, int32_t *__restrict__ start,
                                                           int32_t *__restrict__ end) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    int s = width, e = -1;
    for (int col = 0; col < width; col++) {
        const uint8_t c = code[(size_t)col * (size_t)n_rows + (size_t)r];
        if (c != kGap && c != kDot) {
            if (s == width) s = col;
            e = col;
        }
    }
    start[r] = s;
    end[r] = e;
}

// ---- windows ------------------------------------------------------------------------------------------------------------------------------
struct WinArgs {
    const uint8_t *code;
    const int32_t *start, *end;
    int n_rows, l, skip;
    WinRec *win;
    unsigned long long *cursor;
    long long cap;
    uint64_t *u_words;
    uint32_t *u_cnt, *pairs;
    int pair_stride;
};

struct WinShared { int n_span, n_free, n_dist, n_uniq, n_all, n_pairs, over; long long off; };

// a row's mer at pos: the 5-bit symbols in three words (twelve each), the 2-bit word, and whether it is gap-free
struct Key { uint64_t k0, k1, k2, word; bool gf; };

__device__ inline Key load_key(const WinArgs &a, int r, int pos) {
    Key K{0, 0, 0, 0, true};
    const uint8_t *p = a.code + (size_t)pos * (size_t)a.n_rows + (size_t)r;
    for (int x = 0; x < a.l; x++) {
        uint32_t c = p[(size_t)x * (size_t)a.n_rows];
        if (x == a.l - 1 && c >= 16 && c < kDot) c -= 16;          // only the last byte is upper-cased
        K.gf = K.gf && c < 4;
        K.word = (K.word << 2) | (c & 3);
        if (x < 12) K.k0 = (K.k0 << 5) | c;
        else if (x < 24) K.k1 = (K.k1 << 5) | c;
        else K.k2 = (K.k2 << 5) | c;
    }
    return K;
}

// ascending by key; among equal keys the larger value first, so that padding (value 0) follows a real entry with the padding's key
template <typename KP, typename VP>
__device__ inline void bitonic(KP key, VP val, int n2) {
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = threadIdx.x; x < n2 / 2; x += blockDim.x) {
                const int i = 2 * x - (x & (j - 1)), m = i + j;
                const uint64_t a = key[i], c = key[m];
                const uint32_t va = val[i], vc = val[m];
                const bool after = a > c || (a == c && va < vc);
                if (after == ((i & k) == 0)) { key[i] = c; key[m] = a; val[i] = vc; val[m] = va; }
            }
            __syncthreads();
        }
}

__device__ inline int sort_size(int n) {
    int n2 = kSortMin;
    while (n2 < n) n2 <<= 1;
    return n2;
}

// first / cnt: `slots` table slots (a power of two); skey / sval: room for sort_size(limit) (LDS) or sort_size(n_rows) (global) entries
template <typename FP, typename CP, typename KP, typename VP>
__device__ inline void window_body(const WinArgs &a, int pos, FP first, CP cnt, int slots, int limit, KP skey, VP sval, WinShared &sh) {
    const int t = threadIdx.x, T = blockDim.x;
    for (int x = t; x < slots; x += T) { first[x] = -1; cnt[x] = 0; }
    if (t == 0) { sh.n_span = sh.n_free = sh.n_dist = sh.n_uniq = sh.n_all = sh.n_pairs = sh.over = 0; sh.off = 0; }
    __syncthreads();
    const long long lo = pos, hi = (long long)pos + a.l - 1;
    int my_span = 0, my_free = 0;
    for (int r = t; r < a.n_rows; r += T) {
        if (*(volatile int *)&sh.over) break;
        if ((long long)a.start[r] + a.skip > lo || (long long)a.end[r] - a.skip < hi) continue;
        const Key K = load_key(a, r, pos);
        my_span++;
        my_free += K.gf ? 1 : 0;
        unsigned slot = (unsigned)(mix64(K.k0 ^ mix64(K.k1 ^ mix64(K.k2 + 0x9E3779B97F4A7C15ull))) >> 32) & (unsigned)(slots - 1);
        for (int probe = 0; probe < slots; probe++) {
            int f = *(volatile int32_t *)&first[slot];
            if (f < 0) f = atomicCAS(&first[slot], -1, r);
            if (f < 0) {                       // claimed: r is this mer's first row
                atomicAdd(&cnt[slot], 1u);
                if (atomicAdd(&sh.n_dist, 1) >= limit) *(volatile int *)&sh.over = 1;
                break;
            }
            const Key F = load_key(a, f, pos);
            if (F.k0 == K.k0 && F.k1 == K.k1 && F.k2 == K.k2) { atomicAdd(&cnt[slot], 1u); break; }
            slot = (slot + 1) & (unsigned)(slots - 1);
        }
    }
    atomicAdd(&sh.n_span, my_span);
    atomicAdd(&sh.n_free, my_free);
    __syncthreads();
    if (sh.over) {                             // (the same in every lane) more distinct mers than this table takes
        if (t == 0) a.win[pos] = WinRec{0, 0, -1, 0, 0};
        return;
    }
    // the gap-free entries, sorted by their word
    for (int x = t; x < slots; x += T) {
        const int f = first[x];
        if (f < 0) continue;
        const Key K = load_key(a, f, pos);
        if (K.gf) {
            const int i = atomicAdd(&sh.n_uniq, 1);
            skey[i] = K.word;
            sval[i] = cnt[x];
        }
    }
    __syncthreads();
    const int nu = sh.n_uniq, nd = sh.n_dist;
    int n2 = sort_size(nu);
    for (int x = nu + t; x < n2; x += T) { skey[x] = ~0ull; sval[x] = 0; }
    __syncthreads();
    bitonic(skey, sval, n2);
    if (t == 0) sh.off = (long long)atomicAdd(a.cursor, (unsigned long long)nu);
    __syncthreads();
    const long long off = sh.off;
    if (off + nu <= a.cap)
        for (int x = t; x < nu; x += T) { a.u_words[off + x] = skey[x]; a.u_cnt[off + x] = sval[x]; }
    __syncthreads();
    // the counts of all entries, sorted and run-length coded: (c, m_c)
    for (int x = t; x < slots; x += T)
        if (first[x] >= 0) {
            const int i = atomicAdd(&sh.n_all, 1);
            skey[i] = cnt[x];
            sval[i] = 1;
        }
    n2 = sort_size(nd);
    __syncthreads();
    for (int x = nd + t; x < n2; x += T) { skey[x] = ~0ull; sval[x] = 0; }
    __syncthreads();
    bitonic(skey, sval, n2);
    for (int x = t; x < nd; x += T) {
        const uint64_t c = skey[x];
        if (x > 0 && skey[x - 1] == c) continue;
        int b = x + 1, e = nd;                 // the first index past x whose count differs
        while (b < e) {
            const int mid = (b + e) >> 1;
            if (skey[mid] == c) b = mid + 1; else e = mid;
        }
        const int j = atomicAdd(&sh.n_pairs, 1);
        if (j < a.pair_stride) {
            uint32_t *o = a.pairs + ((size_t)pos * (size_t)a.pair_stride + (size_t)j) * 2;
            o[0] = (uint32_t)c;
            o[1] = (uint32_t)(b - x);
        }
    }
    __syncthreads();
    if (t == 0) a.win[pos] = WinRec{sh.n_span, sh.n_free, nu, sh.n_pairs, off};
}

__global__ __launch_bounds__(kWindowThreads) void dege_window_lds_kernel(WinArgs a) {
    __shared__ int32_t first[kSlots];
    __shared__ uint32_t cnt[kSlots];
    __shared__ uint64_t skey[kSlots];
    __shared__ uint32_t sval[kSlots];
    __shared__ WinShared sh;
    window_body(a, (int)blockIdx.x, first, cnt, kSlots, kLimit, skey, sval, sh);
}

__global__ __launch_bounds__(kWindowThreads) void dege_window_glb_kernel(WinArgs a, const int32_t *__restrict__ list, int32_t *tfirst, uint32_t *tcnt,
                                                                int slots, uint64_t *gkey, uint32_t *gval, int n2cap) {
    __shared__ WinShared sh;
    const size_t b = blockIdx.x;
    window_body(a, list[b], tfirst + b * (size_t)slots, tcnt + b * (size_t)slots, slots, 0x7FFFFFFF, gkey + b * (size_t)n2cap,
                gval + b * (size_t)n2cap, sh);
}

__global__ __launch_bounds__(256) void dege_prefix_kernel(const WinRec *__restrict__ win, const uint32_t *__restrict__ u_cnt,
                                                           uint32_t *__restrict__ u_pre) {
    __shared__ uint32_t part[256];
    const WinRec w = win[blockIdx.x];
    const int t = threadIdx.x, nu = w.n_uniq;
    if (nu <= 0) return;
    const int chunk = (nu + 255) / 256, b = min(nu, t * chunk), e = min(nu, b + chunk);
    uint32_t s = 0;
    for (int x = b; x < e; x++) s += u_cnt[w.off + x];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int x = 0; x < 256; x++) { const uint32_t v = part[x]; part[x] = run; run += v; }
    }
    __syncthreads();
    s = part[t];
    for (int x = b; x < e; x++) { s += u_cnt[w.off + x]; u_pre[w.off + x] = s; }
}

// ---- merging ------------------------------------------------------------------------------------------------------------------------------
struct Planes { uint64_t a, c, g, t; };        // base b in the set of position p: bit 2 (l - 1 - p) of its plane

__device__ inline Planes planes_of(uint64_t m, uint64_t even) {
    const uint64_t lo = m & even, hi = (m >> 1) & even;
    return Planes{~hi & ~lo & even, ~hi & lo, hi & ~lo, hi & lo};
}

// the product of the set sizes, 0xFFFFFFFF when it exceeds 2^31 - 1 (every max_deg is below)
__device__ inline uint32_t degeneracy(const Planes &s) {
    const uint64_t ge2 = (s.a & s.c) | (s.a & s.g) | (s.a & s.t) | (s.c & s.g) | (s.c & s.t) | (s.g & s.t);
    const uint64_t ge3 = (s.a & s.c & s.g) | (s.a & s.c & s.t) | (s.a & s.g & s.t) | (s.c & s.g & s.t);
    const uint64_t all = s.a & s.c & s.g & s.t;
    const int n4 = __popcll(all), n3 = __popcll(ge3) - n4, n2 = __popcll(ge2) - n3 - n4;
    const int sh = n2 + 2 * n4;
    if (sh > 31 || n3 > 19) return 0xFFFFFFFFu;
    uint64_t d = 1;
    for (int x = 0; x < n3; x++) d *= 3;       // 3^19 < 2^31
    d <<= sh;                                  // < 2^62
    return d > 0x7FFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d;
}

__device__ inline void write_rec(int32_t *o, int v0, int v1, int v2, const Planes &s, int l) {
    o[0] = v0; o[1] = v1; o[2] = v2;
    for (int p = 0; p < 32; p++) {
        int m = 0;
        if (p < l) {
            const int b = 2 * (l - 1 - p);
            m = (int)((s.a >> b) & 1) | (int)((s.c >> b) & 1) << 1 | (int)((s.g >> b) & 1) << 2 | (int)((s.t >> b) & 1) << 3;
        }
        o[3 + p] = m;
    }
}

// W / P: the window's nu sorted mers and their inclusive prefix sums (P[nu - 1] = Z)
template <typename WP, typename PP>
__device__ inline void merge_iterations(WP W, PP P, int nu, int pos, int l, uint32_t max_deg, int iters, uint64_t seed, int32_t *iter_out,
                                        int *bm, int *bi, uint32_t *bd, Planes *bp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const uint64_t even = 0x5555555555555555ull & (l == 32 ? ~0ull : ((1ull << (2 * l)) - 1ull));
    int best_m = -1, best_it = 0;
    uint32_t best_d = 0;
    Planes best_s{0, 0, 0, 0};
    for (int it = wave; it < iters; it += n_waves) {
        Planes s{0, 0, 0, 0};
        uint32_t deg = 0, R = P[nu - 1];
        int n_draws = 0;
        int ri0 = 0x7FFFFFFF, ri1 = 0x7FFFFFFF;         // this lane's removed mers: of draw t = lane and of draw t = 64 + lane
        uint32_t rc0 = 0, rc1 = 0;
        for (int t = 0; t < kDraws && deg < max_deg && R > 0; t++) {
            const uint64_t n = ((uint64_t)pos << 24) + ((uint64_t)it << 8) + (uint64_t)t;
            const uint64_t u = mix64(seed + (n + 1) * 0x9E3779B97F4A7C15ull) >> 32;
            const uint32_t r = (uint32_t)((u * (uint64_t)R) >> 32);
            // the smallest i with P[i] - (counts removed at or below i) > r: bisect in P for r + s, s = what was removed at or below the
            // index found for the s before; the index only grows and stops at the answer
            uint32_t rem = 0;
            int i = 0;
            for (int round = 0; round <= kDraws; round++) {
                const uint64_t want = (uint64_t)r + rem;
                int b = 0, e = nu - 1;                  // (P[nu - 1] - all removed = R > r: an answer exists)
                while (b < e) {
                    const int mid = (b + e) >> 1;
                    if ((uint64_t)P[mid] > want) e = mid; else b = mid + 1;
                }
                i = b;
                uint32_t mine = (ri0 <= i ? rc0 : 0u) + (ri1 <= i ? rc1 : 0u);
                for (int sh = 32; sh >= 1; sh >>= 1) mine += __shfl_xor(mine, sh);
                if (mine == rem) break;
                rem = mine;
            }
            const uint32_t ci = P[i] - (i ? P[i - 1] : 0u);
            const uint64_t m = W[i];
            if (lane == (t & 63)) {
                if (t < 64) { ri0 = i; rc0 = ci; } else { ri1 = i; rc1 = ci; }
            }
            R -= ci;
            n_draws++;
            const Planes pm = planes_of(m, even);
            const Planes ns{s.a | pm.a, s.c | pm.c, s.g | pm.g, s.t | pm.t};
            const uint32_t nd = degeneracy(ns);
            if (nd <= max_deg) { s = ns; deg = nd; }
        }
        uint32_t match = 0;
        for (int j = lane; j < nu; j += 64) {
            const Planes pm = planes_of(W[j], even);
            if (((pm.a & s.a) | (pm.c & s.c) | (pm.g & s.g) | (pm.t & s.t)) == even) match += P[j] - (j ? P[j - 1] : 0u);
        }
        for (int sh = 32; sh >= 1; sh >>= 1) match += __shfl_xor(match, sh);
        if (iter_out && lane == 0) write_rec(iter_out + (size_t)it * kRec, (int)deg, (int)match, n_draws, s, l);
        if ((int)match > best_m) { best_m = (int)match; best_it = it; best_d = deg; best_s = s; }       // (its iterations ascend)
    }
    if (lane == 0) { bm[wave] = best_m; bi[wave] = best_it; bd[wave] = best_d; bp[wave] = best_s; }
}

__global__ __launch_bounds__(kMergeThreads) void dege_merge_kernel(const WinRec *__restrict__ win, const int32_t *__restrict__ list,
                                                          const uint64_t *__restrict__ u_words, const uint32_t *__restrict__ u_pre, int l,
                                                          uint32_t max_deg, int iters, uint64_t seed, int32_t *__restrict__ best,
                                                          int32_t *__restrict__ iter_out) {
    __shared__ uint64_t mw[kMergeLds];
    __shared__ uint32_t mpre[kMergeLds];
    __shared__ int bm[kMergeThreads / 64], bi[kMergeThreads / 64];
    __shared__ uint32_t bd[kMergeThreads / 64];
    __shared__ Planes bp[kMergeThreads / 64];
    const int pos = list[blockIdx.x], t = threadIdx.x;
    const WinRec w = win[pos];
    const int nu = w.n_uniq;                   // >= 1: the window is printed
    const uint64_t *gw = u_words + w.off;
    const uint32_t *gp = u_pre + w.off;
    if (nu <= kMergeLds) {
        for (int x = t; x < nu; x += kMergeThreads) { mw[x] = gw[x]; mpre[x] = gp[x]; }
        __syncthreads();
        merge_iterations(mw, mpre, nu, pos, l, max_deg, iters, seed, iter_out, bm, bi, bd, bp);
    } else {
        merge_iterations(gw, gp, nu, pos, l, max_deg, iters, seed, iter_out, bm, bi, bd, bp);
    }
    __syncthreads();
    if (t == 0) {
        int k = -1;
        for (int x = 0; x < kMergeThreads / 64; x++)
            if (bm[x] >= 0 && (k < 0 || bm[x] > bm[k] || (bm[x] == bm[k] && bi[x] < bi[k]))) k = x;
        if (k >= 0) write_rec(best + (size_t)pos * kRec, bm[k], (int)bd[k], bi[k], bp[k], l);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
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

void fill_lut(uint8_t *lut) {
    memset(lut, kBad, 256);
    static const char letters[] = "ACGTRYSWKMBDHVN";     // codes 0 .. 14, lower case 16 .. 30
    for (int i = 0; i < 15; i++) {
        lut[(uint8_t)letters[i]] = (uint8_t)i;
        lut[(uint8_t)(letters[i] + 32)] = (uint8_t)(16 + i);
    }
    lut[(uint8_t)'-'] = kGap;
    lut[(uint8_t)'.'] = kDot;
}

void free_windows_of(mp_ctx *c, DegeState *s) {
    dev_free(c, &s->win, (size_t)s->n_win);
    dev_free(c, &s->u_words, (size_t)s->u_cap);
    dev_free(c, &s->u_cnt, (size_t)s->u_cap);
    dev_free(c, &s->u_pre, (size_t)s->u_cap);
    dev_free(c, &s->pairs, (size_t)s->n_win * (size_t)s->pair_stride * 2);
    dev_free(c, &s->best, (size_t)s->n_win * kRec);
    dev_free(c, &s->list, (size_t)s->n_printed);
    s->n_win = s->n_printed = 0;
    s->u_cap = s->u_total = 0;
    s->l = 0;
    s->merged = false;
    s->h_win.clear();
    s->h_entropy.clear();
}

// One pass over every window at the capacity s->u_cap: the LDS kernel, then the windows it gave up in batches on the global tables.
// Leaves the records in s->h_win and the entries needed in *total.
int window_pass(mp_ctx *c, DegeState *s, unsigned long long *d_cursor, long long *total) {
    static const char *who = "mp_dege_windows";
    WinArgs a{s->code, s->start, s->end, s->n_rows, s->l, s->skip, s->win, d_cursor, s->u_cap, s->u_words, s->u_cnt, s->pairs, s->pair_stride};
    int rc;
    if ((rc = dev(c, hipMemsetAsync(d_cursor, 0, sizeof(unsigned long long), c->stream), who, "hipMemsetAsync"))) return rc;
    hipLaunchKernelGGL(dege_window_lds_kernel, dim3((unsigned)s->n_win), dim3(kWindowThreads), 0, c->stream, a);
    if ((rc = dev(c, hipGetLastError(), who, "dege_window_lds_kernel"))) return rc;
    s->h_win.resize((size_t)s->n_win);
    if ((rc = dev(c, hipMemcpyAsync(s->h_win.data(), s->win, sizeof(WinRec) * (size_t)s->n_win, hipMemcpyDeviceToHost, c->stream), who, "copy"))) return rc;
    if ((rc = dev(c, hipStreamSynchronize(c->stream), who, "hipStreamSynchronize"))) return rc;
    std::vector<int32_t> over;
    for (int32_t w = 0; w < s->n_win; w++)
        if (s->h_win[(size_t)w].n_uniq < 0) over.push_back(w);
    s->n_global = (int64_t)over.size();
    if (!over.empty()) {
        int slots = 2 * kSlots, n2cap = kSortMin;
        while (slots < 2 * (long long)s->n_rows) slots <<= 1;          // n_rows < 2^30 (mp_dege_load)
        while (n2cap < s->n_rows) n2cap <<= 1;
        const size_t per = (size_t)slots * 8 + (size_t)n2cap * 12;
        const size_t batch = std::max<size_t>(1, std::min<size_t>(over.size(), ((size_t)256 << 20) / per));
        int32_t *d_list = nullptr, *tfirst = nullptr;
        uint32_t *tcnt = nullptr, *gval = nullptr;
        uint64_t *gkey = nullptr;
        if ((rc = dev_alloc(c, &d_list, over.size())) == MP_OK && (rc = dev_alloc(c, &tfirst, batch * (size_t)slots)) == MP_OK &&
            (rc = dev_alloc(c, &tcnt, batch * (size_t)slots)) == MP_OK && (rc = dev_alloc(c, &gkey, batch * (size_t)n2cap)) == MP_OK &&
            (rc = dev_alloc(c, &gval, batch * (size_t)n2cap)) == MP_OK &&
            (rc = dev(c, hipMemcpyAsync(d_list, over.data(), sizeof(int32_t) * over.size(), hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK)
            for (size_t at = 0; at < over.size() && rc == MP_OK; at += batch) {
                const size_t nb = std::min(batch, over.size() - at);
                hipLaunchKernelGGL(dege_window_glb_kernel, dim3((unsigned)nb), dim3(kWindowThreads), 0, c->stream, a, (const int32_t *)(d_list + at), tfirst, tcnt,
                                   slots, gkey, gval, n2cap);
                rc = dev(c, hipGetLastError(), who, "dege_window_glb_kernel");
            }
        if (rc == MP_OK) rc = dev(c, hipMemcpyAsync(s->h_win.data(), s->win, sizeof(WinRec) * (size_t)s->n_win, hipMemcpyDeviceToHost, c->stream), who, "copy");
        (void)hipStreamSynchronize(c->stream);
        dev_free(c, &d_list, over.size()); dev_free(c, &tfirst, batch * (size_t)slots); dev_free(c, &tcnt, batch * (size_t)slots);
        dev_free(c, &gkey, batch * (size_t)n2cap); dev_free(c, &gval, batch * (size_t)n2cap);
        if (rc) return rc;
    }
    unsigned long long cur = 0;
    if ((rc = dev(c, hipMemcpy(&cur, d_cursor, sizeof cur, hipMemcpyDeviceToHost), who, "copy"))) return rc;
    *total = (long long)cur;
    return MP_OK;
}

int launch_merge(mp_ctx *c, DegeState *s, const int32_t *d_list, int n, int32_t *best, int32_t *iter_out, const char *who) {
    hipLaunchKernelGGL(dege_merge_kernel, dim3((unsigned)n), dim3(kMergeThreads), 0, c->stream, (const WinRec *)s->win, d_list, (const uint64_t *)s->u_words,
                       (const uint32_t *)s->u_pre, (int)s->l, (uint32_t)s->max_deg, (int)s->iters, s->seed, best, iter_out);
    return dev(c, hipGetLastError(), who, "dege_merge_kernel");
}

}  // namespace

void free_dege(mp_ctx *c) {
    DegeState *s = c->dege;
    if (!s) return;
    free_windows_of(c, s);
    dev_free(c, &s->code, (size_t)s->n_rows * (size_t)s->width);
    dev_free(c, &s->start, (size_t)s->n_rows);
    dev_free(c, &s->end, (size_t)s->n_rows);
    delete s;
    c->dege = nullptr;
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_dege_load(mp_ctx *c, int32_t n_rows, int32_t width, const uint8_t *bytes) {
    static const char *who = "mp_dege_load";
    if (!c) return MP_ERR_ARG;
    if (n_rows < 1 || width < 1 || !bytes) return fail(c, MP_ERR_ARG, "%s: bad arguments", who);
    const long long total = (long long)n_rows * width;
    if (n_rows >= (1 << 30) || total > (1LL << 40)) return fail(c, MP_ERR_ARG, "%s: %d rows of %d columns are beyond the limit", who, n_rows, width);
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    free_dege(c);
    DegeState *s = c->dege = new DegeState;
    s->n_rows = n_rows;
    s->width = width;
    uint8_t lut[256];
    fill_lut(lut);
    uint8_t *d_raw = nullptr, *d_lut = nullptr;
    unsigned long long *d_bad = nullptr, bad = kNoBad;
    int rc;
    if ((rc = dev_alloc(c, &s->code, (size_t)total)) == MP_OK && (rc = dev_alloc(c, &s->start, (size_t)n_rows)) == MP_OK &&
        (rc = dev_alloc(c, &s->end, (size_t)n_rows)) == MP_OK && (rc = dev_alloc(c, &d_raw, (size_t)total)) == MP_OK &&
        (rc = dev_alloc(c, &d_lut, (size_t)256)) == MP_OK && (rc = dev_alloc(c, &d_bad, (size_t)1)) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_raw, bytes, (size_t)total, hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_lut, lut, sizeof lut, hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_bad, &bad, sizeof bad, hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK) {
        const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 1 << 20);
        hipLaunchKernelGGL(dege_code_kernel, dim3(grid), dim3(256), 0, c->stream, (const uint8_t *)d_raw, (const uint8_t *)d_lut, total, (int)n_rows,
                           (int)width, s->code, d_bad);
        if ((rc = dev(c, hipGetLastError(), who, "dege_code_kernel")) == MP_OK) {
            hipLaunchKernelGGL(dege_extent_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)s->code, (int)n_rows,
                               (int)width, s->start, s->end);
            if ((rc = dev(c, hipGetLastError(), who, "dege_extent_kernel")) == MP_OK)
                rc = dev(c, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, c->stream), who, "copy");
        }
    }
    if (rc == MP_OK) rc = dev(c, hipStreamSynchronize(c->stream), who, "hipStreamSynchronize"); else (void)hipStreamSynchronize(c->stream);
    dev_free(c, &d_raw, (size_t)total); dev_free(c, &d_lut, (size_t)256); dev_free(c, &d_bad, (size_t)1);
    if (rc == MP_OK && bad != kNoBad)
        rc = fail(c, MP_ERR_ARG, "%s: row %lld, column %lld: byte 0x%02X is no IUPAC nucleotide letter, '-' or '.'", who, (long long)(bad / (unsigned long long)width),
                  (long long)(bad % (unsigned long long)width), (unsigned)bytes[bad]);
    if (rc) free_dege(c);
    return rc;
}

int mp_dege_windows(mp_ctx *c, int32_t l, int32_t skip, int32_t depth, int32_t *n_windows) {
    static const char *who = "mp_dege_windows";
    if (!c) return MP_ERR_ARG;
    DegeState *s = c->dege;
    if (!s) return fail(c, MP_ERR_ARG, "%s: no alignment (mp_dege_load first)", who);
    if (l < MP_DEGE_MIN_L || l > MP_DEGE_MAX_L) return fail(c, MP_ERR_ARG, "%s: primer length %d (%d..%d)", who, l, MP_DEGE_MIN_L, MP_DEGE_MAX_L);
    if (skip < 0 || depth < 1) return fail(c, MP_ERR_ARG, "%s: skip %d (>= 0), depth %d (>= 1)", who, skip, depth);
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    free_windows_of(c, s);
    s->ms[0] = s->ms[1] = 0;
    s->n_global = 0;
    s->l = l; s->skip = skip; s->depth = depth;
    s->n_win = s->width >= l ? s->width - l + 1 : 0;
    if (n_windows) *n_windows = s->n_win;
    if (s->n_win == 0) return MP_OK;
    // distinct count values c_1 < c_2 < .. of a window sum to at most n_rows: fewer than sqrt(2 n_rows) + 1 of them
    s->pair_stride = (int32_t)std::min<double>((double)s->n_rows, std::floor(std::sqrt(2.0 * s->n_rows)) + 1);
    s->u_cap = std::min<long long>((long long)s->n_win * std::min<long long>(kLimit, s->n_rows), 8LL << 20);
    unsigned long long *d_cursor = nullptr;
    long long total = 0;
    int rc;
    if ((rc = dev_alloc(c, &s->win, (size_t)s->n_win)) == MP_OK && (rc = dev_alloc(c, &s->pairs, (size_t)s->n_win * (size_t)s->pair_stride * 2)) == MP_OK &&
        (rc = dev_alloc(c, &d_cursor, (size_t)1)) == MP_OK)
        for (int attempt = 0; attempt < 2 && rc == MP_OK; attempt++) {     // the second time with the capacity the first one asked for
            if ((rc = dev_alloc(c, &s->u_words, (size_t)s->u_cap)) || (rc = dev_alloc(c, &s->u_cnt, (size_t)s->u_cap)) ||
                (rc = dev_alloc(c, &s->u_pre, (size_t)s->u_cap)))
                break;
            if (attempt == 1) s->ms[0] = 0;
            rc = timed(c, who, &s->ms[0], [&]() {
                int rc2 = window_pass(c, s, d_cursor, &total);
                if (rc2 == MP_OK && total <= s->u_cap) {
                    hipLaunchKernelGGL(dege_prefix_kernel, dim3((unsigned)s->n_win), dim3(256), 0, c->stream, (const WinRec *)s->win, (const uint32_t *)s->u_cnt,
                                       s->u_pre);
                    rc2 = dev(c, hipGetLastError(), who, "dege_prefix_kernel");
                }
                return rc2;
            });
            if (rc || total <= s->u_cap) break;
            dev_free(c, &s->u_words, (size_t)s->u_cap); dev_free(c, &s->u_cnt, (size_t)s->u_cap); dev_free(c, &s->u_pre, (size_t)s->u_cap);
            s->u_cap = total;
        }
    dev_free(c, &d_cursor, (size_t)1);
    // the entropy, on the host, from the pairs (c, m_c) in ascending c (the rule of mprime_dege.h)
    std::vector<uint32_t> pairs;
    if (rc == MP_OK) {
        pairs.resize((size_t)s->n_win * (size_t)s->pair_stride * 2);
        rc = dev(c, hipMemcpy(pairs.data(), s->pairs, sizeof(uint32_t) * pairs.size(), hipMemcpyDeviceToHost), who, "copy");
    }
    if (rc == MP_OK) {
        s->h_entropy.assign((size_t)s->n_win, 0.0);
        const double log2 = std::log(2.0);
        std::vector<std::pair<uint32_t, uint32_t>> v;
        for (int32_t w = 0; w < s->n_win && rc == MP_OK; w++) {
            const WinRec &r = s->h_win[(size_t)w];
            if (r.n_pairs > s->pair_stride) { rc = fail(c, MP_ERR_DEVICE, "%s: window %d has %d count values (%d expected at the most)", who, w, r.n_pairs, s->pair_stride); break; }
            v.clear();
            for (int32_t x = 0; x < r.n_pairs; x++) {
                const uint32_t *p = pairs.data() + ((size_t)w * (size_t)s->pair_stride + (size_t)x) * 2;
                v.emplace_back(p[0], p[1]);
            }
            std::sort(v.begin(), v.end());
            double e = 0;
            for (auto &p : v) {
                const double x = (double)p.first / (double)r.n_span;
                e = e - (double)p.second * (x * std::log(x) / log2);
            }
            s->h_entropy[(size_t)w] = e;
        }
    }
    if (rc) { free_windows_of(c, s); return rc; }
    s->u_total = total;
    return MP_OK;
}

int mp_dege_window_table(mp_ctx *c, int32_t *nums, double *entropy) {
    if (!c) return MP_ERR_ARG;
    DegeState *s = c->dege;
    if (!s || s->l == 0) return fail(c, MP_ERR_ARG, "mp_dege_window_table: no windows (mp_dege_windows first)");
    if (s->n_win && (!nums || !entropy)) return fail(c, MP_ERR_ARG, "mp_dege_window_table: null argument");
    for (int32_t w = 0; w < s->n_win; w++) {
        const WinRec &r = s->h_win[(size_t)w];
        int32_t *o = nums + (size_t)w * MP_DEGE_WIN;
        o[0] = r.n_span; o[1] = r.n_free; o[2] = r.n_uniq; o[3] = r.n_free >= s->depth ? 1 : 0;
        entropy[w] = s->h_entropy[(size_t)w];
    }
    return MP_OK;
}

int mp_dege_unique(mp_ctx *c, int32_t pos, int64_t cap, uint64_t *words, int32_t *counts) {
    static const char *who = "mp_dege_unique";
    if (!c) return MP_ERR_ARG;
    DegeState *s = c->dege;
    if (!s || s->l == 0) return fail(c, MP_ERR_ARG, "%s: no windows (mp_dege_windows first)", who);
    if (pos < 0 || pos >= s->n_win) return fail(c, MP_ERR_ARG, "%s: window %d of %d", who, pos, s->n_win);
    const WinRec &r = s->h_win[(size_t)pos];
    if (cap < r.n_uniq) return fail(c, MP_ERR_CAPACITY, "%s: window %d has %d unique mers, room for %lld", who, pos, r.n_uniq, (long long)cap);
    if (r.n_uniq == 0) return MP_OK;
    if (!words || !counts) return fail(c, MP_ERR_ARG, "%s: null argument", who);
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipMemcpy(words, s->u_words + r.off, sizeof(uint64_t) * (size_t)r.n_uniq, hipMemcpyDeviceToHost));
    HIPCK(c, hipMemcpy(counts, s->u_cnt + r.off, sizeof(uint32_t) * (size_t)r.n_uniq, hipMemcpyDeviceToHost));
    return MP_OK;
}

int mp_dege_merge(mp_ctx *c, int32_t max_deg, int32_t iters, uint64_t seed) {
    static const char *who = "mp_dege_merge";
    if (!c) return MP_ERR_ARG;
    DegeState *s = c->dege;
    if (!s || s->l == 0) return fail(c, MP_ERR_ARG, "%s: no windows (mp_dege_windows first)", who);
    if (max_deg < 1) return fail(c, MP_ERR_ARG, "%s: maximum degeneracy %d (1..2147483647)", who, max_deg);
    if (iters < 1 || iters > MP_DEGE_MAX_ITERS) return fail(c, MP_ERR_ARG, "%s: %d iterations (1..%d)", who, iters, MP_DEGE_MAX_ITERS);
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    dev_free(c, &s->best, (size_t)s->n_win * kRec);
    dev_free(c, &s->list, (size_t)s->n_printed);
    s->merged = false;
    s->max_deg = max_deg; s->iters = iters; s->seed = seed;
    s->ms[1] = 0;
    std::vector<int32_t> list;
    for (int32_t w = 0; w < s->n_win; w++)
        if (s->h_win[(size_t)w].n_free >= s->depth) list.push_back(w);
    s->n_printed = (int32_t)list.size();
    if (s->n_win == 0) { s->merged = true; return MP_OK; }
    int rc;
    if ((rc = dev_alloc(c, &s->best, (size_t)s->n_win * kRec)) == MP_OK && (rc = dev_alloc(c, &s->list, list.size())) == MP_OK &&
        (rc = dev(c, hipMemsetAsync(s->best, 0xFF, sizeof(int32_t) * (size_t)s->n_win * kRec, c->stream), who, "hipMemsetAsync")) == MP_OK &&
        (list.empty() || (rc = dev(c, hipMemcpyAsync(s->list, list.data(), sizeof(int32_t) * list.size(), hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK) &&
        !list.empty())
        rc = timed(c, who, &s->ms[1], [&]() { return launch_merge(c, s, s->list, s->n_printed, s->best, nullptr, who); });
    if (rc == MP_OK) rc = dev(c, hipStreamSynchronize(c->stream), who, "hipStreamSynchronize");
    if (rc) return rc;
    s->merged = true;
    return MP_OK;
}

int mp_dege_best(mp_ctx *c, int32_t *out) {
    if (!c) return MP_ERR_ARG;
    DegeState *s = c->dege;
    if (!s || !s->merged) return fail(c, MP_ERR_ARG, "mp_dege_best: no result (mp_dege_merge first)");
    if (s->n_win == 0) return MP_OK;
    if (!out) return fail(c, MP_ERR_ARG, "mp_dege_best: null argument");
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    HIPCK(c, hipMemcpy(out, s->best, sizeof(int32_t) * (size_t)s->n_win * kRec, hipMemcpyDeviceToHost));
    return MP_OK;
}

int mp_dege_iterations(mp_ctx *c, int32_t pos, int32_t *out) {
    static const char *who = "mp_dege_iterations";
    if (!c) return MP_ERR_ARG;
    DegeState *s = c->dege;
    if (!s || !s->merged) return fail(c, MP_ERR_ARG, "%s: no result (mp_dege_merge first)", who);
    if (pos < 0 || pos >= s->n_win || !out) return fail(c, MP_ERR_ARG, "%s: window %d of %d", who, pos, s->n_win);
    if (s->h_win[(size_t)pos].n_free < s->depth) return fail(c, MP_ERR_ARG, "%s: window %d is not printed", who, pos);
    HIPCK(c, hipSetDevice(c->dev));
    int32_t *d_pos = nullptr, *d_out = nullptr, *scratch = nullptr;
    const size_t n = (size_t)s->iters * kRec;
    int rc;
    // the kernel writes the window's winner too: into a scratch table, so that the result of mp_dege_merge stays what it is
    if ((rc = dev_alloc(c, &d_pos, (size_t)1)) == MP_OK && (rc = dev_alloc(c, &d_out, n)) == MP_OK && (rc = dev_alloc(c, &scratch, (size_t)s->n_win * kRec)) == MP_OK &&
        (rc = dev(c, hipMemcpyAsync(d_pos, &pos, sizeof pos, hipMemcpyHostToDevice, c->stream), who, "copy")) == MP_OK) {
        rc = launch_merge(c, s, d_pos, 1, scratch, d_out, who);
        if (rc == MP_OK) rc = dev(c, hipMemcpyAsync(out, d_out, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream), who, "copy");
    }
    if (rc == MP_OK) rc = dev(c, hipStreamSynchronize(c->stream), who, "hipStreamSynchronize"); else (void)hipStreamSynchronize(c->stream);
    dev_free(c, &d_pos, (size_t)1); dev_free(c, &d_out, n); dev_free(c, &scratch, (size_t)s->n_win * kRec);
    return rc;
}

int mp_dege_stats(mp_ctx *c, double *ms, int64_t *counts) {
    if (!c) return MP_ERR_ARG;
    DegeState *s = c->dege;
    if (ms) { ms[0] = s ? s->ms[0] : 0; ms[1] = s ? s->ms[1] : 0; }
    if (counts) {
        counts[0] = s ? s->n_win : 0;
        counts[1] = s ? s->n_printed : 0;
        counts[2] = s ? s->u_total : 0;
        counts[3] = s ? s->n_global : 0;
    }
    return MP_OK;
}

}  // extern "C"
