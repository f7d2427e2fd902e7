// anchor.hip — anchored alignment (include/mprime_anchor.h): every query is placed on the anchor of a seed alignment by a banded
// affine-gap (Gotoh) alignment around a voted seed diagonal.  Three kernels per batch of queries:
//   anchor_vote_kernel   one wavefront per query: its 12-mers are looked up in the anchor's open-addressing table, the votes per
//                        diagonal counted in an LDS histogram (two 16-bit counters per word), d0 chosen by a wave reduction
//   anchor_dp_kernel     one wavefront per query, lanes own the band's diagonals (R = 1, 2, 4 or 8 neighbouring diagonals per lane for
//                        2W + 1 <= 64 R).  ANTI-DIAGONAL sweep: at step s the cells with i + j = s are computed; cell (i, j) on diagonal
//                        d reads its left cell (i, j-1) from diagonal d - 1 and its upper cell (i-1, j) from diagonal d + 1, both
//                        computed at step s - 1, and its diagonal cell from its own registers — no dependency inside a step, so no
//                        scan; a lane is busy every other step.  Four predecessor bits per cell (H source 2, E opened, F opened)
//                        are collected eight rows to a word per diagonal and stored to the traceback buffer in HBM.  Anchor codes
//                        (shared by the workgroup's waves) and the wave's query codes sit in LDS; the pair score is two compares on
//                        the codes, so no per-letter profile rows are kept.
//   anchor_trace_kernel  one lane per query walks the bits from the end cell (a chain of dependent loads: latency-bound, so it
//                        gets its parallelism from the number of queries), writes the letters in anchor space, the meta record and the ops
//   anchor_emit_kernel   expands anchor space to the seed's L columns: 16 row bytes per lane, one 128-bit store each
#include "common.hpp"
#include "seedword.hpp"
#include "../../include/mprime_anchor.h"

namespace mp {

namespace {

constexpr int kNeg = -(1 << 30);               // "no such cell": below every real score by more than any real score can gain
constexpr int kNoPath = -(3 << 28);            // a best end score below this was never fed by row 0 (mprime_anchor.h: MP_ANCHOR_MAX_PARAM)
constexpr int kWord = MP_ANCHOR_WORD;

__host__ __device__ inline uint8_t upper_letter(uint8_t ch) { return ch >= 'a' && ch <= 'z' ? (uint8_t)(ch - 32) : ch; }

// ---- votes --------------------------------------------------------------------------------------------------------------------------
// better(a, b): diagonal vote (ca, da) beats (cb, db) — more votes, then the smaller |d|, then the smaller d
__device__ inline bool vote_better(int ca, int da, int cb, int db) {
    if (ca != cb) return ca > cb;
    const int aa = da < 0 ? -da : da, ab = db < 0 ? -db : db;
    if (aa != ab) return aa < ab;
    return da < db;
}

__global__ __launch_bounds__(64) void anchor_vote_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ off, int n,
                                                          const uint32_t *__restrict__ akmer, const int32_t *__restrict__ table, int log2_slots,
                                                          int32_t *__restrict__ d0_out) {
    extern __shared__ uint32_t hist[];         // bin b = d + m (1 .. m + n - 1): counter (b & 1) of word b >> 1
    const int q = blockIdx.x, lane = threadIdx.x;
    const uint8_t *qb = bytes + off[q];
    const int m = (int)(off[q + 1] - off[q]);
    const int words = (m + n) / 2 + 1;
    for (int x = lane; x < words; x += 64) hist[x] = 0;
    __syncthreads();
    const uint32_t mask = (1u << log2_slots) - 1;
    for (int i = lane; i + kWord <= m && n >= kWord; i += 64) {
        uint32_t kmer = 0;
        bool ok = true;
        for (int x = 0; x < kWord; x++) {
            const int cd = base_code(qb[i + x]);
            ok = ok && cd < 4;
            kmer = (kmer << 2) | (uint32_t)(cd & 3);
        }
        if (!ok) continue;
        uint32_t slot = word_hash(kmer, log2_slots);
        for (int32_t j; (j = table[slot]) >= 0; slot = (slot + 1) & mask)
            if (akmer[j] == kmer) {
                const int b = j - i + m;
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
    if (lane == 0) d0_out[q] = best_c > 0 ? best_d : min(max(0, -m), n);
}

// ---- the banded Gotoh sweep ----------------------------------------------------------------------------------------------------------
// Traceback bits of cell (i, t), i = 1 .. m, t = diagonal index inside the band: nibble (i - 1) & 7 of word tb[tb_off[q] + ((i - 1) >> 3) *
// 64 R + t]; bits 0-1: H came from 0 the diagonal, 1 E, 2 F (3: the cell lies outside the matrix); bit 2: E opened here; bit 3: F opened here.
template <int R>
__global__ __launch_bounds__(256) void anchor_dp_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ off, int nq,
                                                         const int32_t *__restrict__ d0v, const uint8_t *__restrict__ acode, int n, int W, int match,
                                                         int mismatch, int open_ext, int ext, int mstride, uint32_t *__restrict__ tb,
                                                         const int64_t *__restrict__ tb_off, int32_t *__restrict__ end_out) {
    extern __shared__ uint8_t lds[];           // [npad] anchor codes, then [mstride] query codes per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    const int npad = (n + 15) & ~15;
    for (int x = threadIdx.x; x < n; x += blockDim.x) lds[x] = acode[x];
    const int q = blockIdx.x * wpb + wave;
    uint8_t *qc = lds + npad + wave * mstride;
    int m = 0;
    if (q < nq) {
        const uint8_t *qb = bytes + off[q];
        m = (int)(off[q + 1] - off[q]);
        for (int x = lane; x < m; x += 64) qc[x] = (uint8_t)base_code(qb[x]);
    }
    __syncthreads();                           // (the only barrier: what follows is per wave)
    if (q >= nq) return;
    const int B = 2 * W + 1, dlo = d0v[q] - W, Bpad = 64 * R;
    uint32_t *tbq = tb + tb_off[q];
    int H[R], E[R], F[R];
    uint32_t acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int t = lane * R + r, d = dlo + t;
        H[r] = (t < B && d >= 0 && d <= n) ? 0 : kNeg;          // the row-0 cell of the diagonal
        E[r] = F[r] = kNeg;
        acc[r] = 0;
    }
    const int s_end = 2 * m + dlo + B - 1;
    for (int s = 2 + dlo; s <= s_end; s++) {
        // the neighbouring lanes' edge diagonals as of step s - 1
        int hl_edge = __shfl_up(H[R - 1], 1), el_edge = __shfl_up(E[R - 1], 1);
        int hu_edge = __shfl_down(H[0], 1), fu_edge = __shfl_down(F[0], 1);
        if (lane == 0) hl_edge = el_edge = kNeg;
        if (lane == 63) hu_edge = fu_edge = kNeg;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int t = lane * R + r, d = dlo + t, two_i = s - d;
            if ((two_i & 1) || two_i < 2 || two_i > 2 * m || t >= B) continue;       // (the cells of one step have one parity: H[r +- 1] are of step s - 1)
            const int i = two_i >> 1, j = i + d;
            int h = kNeg, e = kNeg, f = kNeg;
            uint32_t bits = 3;
            if (j >= 0 && j <= n) {
                const int hl = r > 0 ? H[r > 0 ? r - 1 : 0] : hl_edge, el = r > 0 ? E[r > 0 ? r - 1 : 0] : el_edge;
                const int hu = r < R - 1 ? H[r < R - 1 ? r + 1 : 0] : hu_edge, fu = r < R - 1 ? F[r < R - 1 ? r + 1 : 0] : fu_edge;
                const int eo = hl - open_ext, ee = el - ext, fo = hu - open_ext, fe = fu - ext;
                e = max(eo, ee);
                f = max(fo, fe);
                int dg = kNeg;
                if (j >= 1) {
                    const int qcd = qc[i - 1], acd = lds[j - 1];
                    dg = H[r] + ((qcd < 4 && acd < 4) ? (qcd == acd ? match : -mismatch) : 0);
                }
                h = max(dg, max(e, f));
                bits = (dg >= e && dg >= f) ? 0u : (e >= f ? 1u : 2u);
                bits |= (eo >= ee ? 4u : 0u) | (fo >= fe ? 8u : 0u);
                h = max(h, kNeg); e = max(e, kNeg); f = max(f, kNeg);
            }
            H[r] = h; E[r] = e; F[r] = f;
            const int k = i - 1;
            acc[r] |= bits << (4 * (k & 7));
            if ((k & 7) == 7 || i == m) {
                tbq[(size_t)(k >> 3) * Bpad + t] = acc[r];
                acc[r] = 0;
            }
        }
    }
    // the end cell: the largest H(m, j) of the band, the smallest j (= the smallest t) among equals
    int best = kNeg, best_t = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int t = lane * R + r;
        if (t < B && H[r] > best) { best = H[r]; best_t = t; }
    }
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const int ob = __shfl_xor(best, sh), ot = __shfl_xor(best_t, sh);
        if (ob > best || (ob == best && ot < best_t)) { best = ob; best_t = ot; }
    }
    if (lane == 0) {
        const bool none = best < kNoPath;
        end_out[2 * q] = none ? MP_ANCHOR_NO_SCORE : best;
        end_out[2 * q + 1] = none ? -1 : best_t;
    }
}

// ---- traceback ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void anchor_trace_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ off, int nq,
                                                           const int32_t *__restrict__ d0v, const uint8_t *__restrict__ acode,
                                                           const int32_t *__restrict__ col, int n, int W, int R, int permille,
                                                           const uint32_t *__restrict__ tb, const int64_t *__restrict__ tb_off,
                                                           const int32_t *__restrict__ end_in, uint8_t *__restrict__ arow, int32_t *__restrict__ meta,
                                                           uint8_t *__restrict__ ops, const int64_t *__restrict__ ops_off) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= nq) return;
    const uint8_t *qb = bytes + off[q];
    const int m = (int)(off[q + 1] - off[q]), d0 = d0v[q], dlo = d0 - W, B = 2 * W + 1, Bpad = 64 * R;
    const uint32_t *tbq = tb + tb_off[q];
    uint8_t *ar = arow + (size_t)q * n;
    int32_t *mt = meta + (size_t)q * MP_ANCHOR_META;
    const int score = end_in[2 * q];
    int t = end_in[2 * q + 1];
    int n_match = 0, n_ins = 0, n_del = 0, j_first = -1, j_last = -1, status = 0;
    if (t < 0) status = 3;
    else {
        uint8_t *op = ops ? ops + ops_off[q + 1] : nullptr;
        int i = m, state = 0;
        bool touch = false;
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
            }
        }
        if (touch) status |= 2;
        if ((long long)n_match * 1000 < (long long)permille * m) status |= 1;
    }
    mt[0] = score; mt[1] = d0; mt[2] = n_match; mt[3] = n_ins; mt[4] = n_del;
    mt[5] = j_first >= 0 ? col[j_first] : -1;
    mt[6] = j_last >= 0 ? col[j_last] : -1;
    mt[7] = status; mt[8] = j_first; mt[9] = j_last;
}

// rows [nq][L] as one run of bytes: lane g writes bytes 16 g .. 16 g + 15 (the buffer starts on a hipMalloc boundary)
__global__ __launch_bounds__(256) void anchor_emit_kernel(const uint8_t *__restrict__ arow, const int32_t *__restrict__ meta,
                                                           const int32_t *__restrict__ colinv, int n, int L, long long total,
                                                           uint8_t *__restrict__ rows) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x, b0 = g * 16;
    if (b0 >= total) return;
    long long q = b0 / L;
    int c = (int)(b0 - q * L);
    int jf = meta[q * MP_ANCHOR_META + 8], jl = meta[q * MP_ANCHOR_META + 9];
    uint32_t w[4] = {0, 0, 0, 0};
    const int cnt = (int)min(16LL, total - b0);
#pragma unroll
    for (int x = 0; x < 16; x++) {
        uint8_t ch = '-';
        if (x < cnt) {
            const int j = colinv[c];
            if (j >= jf && j <= jl && j >= 0) ch = arow[(size_t)q * n + j];
            if (++c == L) {
                c = 0;
                q++;
                if (x + 1 < cnt) { jf = meta[q * MP_ANCHOR_META + 8]; jl = meta[q * MP_ANCHOR_META + 9]; }
            }
        }
        w[x >> 2] |= (uint32_t)ch << (8 * (x & 3));
    }
    if (cnt == 16) *reinterpret_cast<uint4 *>(rows + b0) = make_uint4(w[0], w[1], w[2], w[3]);
    else
        for (int x = 0; x < cnt; x++) rows[b0 + x] = (uint8_t)(w[x >> 2] >> (8 * (x & 3)));
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

void free_anchor(mp_ctx *c) {
    dev_free(c, &c->an_code, (size_t)c->an_n);
    dev_free(c, &c->an_kmer, (size_t)c->an_n);
    dev_free(c, &c->an_table, (size_t)c->an_slots);
    dev_free(c, &c->an_col, (size_t)c->an_n);
    dev_free(c, &c->an_colinv, (size_t)c->an_L);
    c->an_n = c->an_L = c->an_slots = 0;
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_anchor_set(mp_ctx *c, const uint8_t *codes, int32_t n, const int32_t *col, int32_t L, const mp_anchor_params *p) {
    if (!c) return MP_ERR_ARG;
    if (!codes || !col || !p) return fail(c, MP_ERR_ARG, "mp_anchor_set: null argument");
    if (n < 1 || n > MP_ANCHOR_MAX_LEN) return fail(c, MP_ERR_ARG, "mp_anchor_set: anchor of %d positions (1..%d)", n, MP_ANCHOR_MAX_LEN);
    if (L < n) return fail(c, MP_ERR_ARG, "mp_anchor_set: %d columns for %d anchor positions", L, n);
    const int32_t par[6] = {p->match, p->mismatch, p->gap_open, p->gap_extend, p->band, p->min_identity_permille};
    for (int i = 0; i < 4; i++)
        if (par[i] < 0 || par[i] > MP_ANCHOR_MAX_PARAM) return fail(c, MP_ERR_ARG, "mp_anchor_set: score parameter %d (0..%d)", par[i], MP_ANCHOR_MAX_PARAM);
    if (par[4] < 0 || par[4] > MP_ANCHOR_MAX_BAND) return fail(c, MP_ERR_ARG, "mp_anchor_set: band %d (0..%d)", par[4], MP_ANCHOR_MAX_BAND);
    if (par[5] < 0 || par[5] > 1000) return fail(c, MP_ERR_ARG, "mp_anchor_set: min_identity_permille %d (0..1000)", par[5]);
    for (int32_t j = 0; j < n; j++)
        if (col[j] < 0 || col[j] >= L || (j && col[j] <= col[j - 1])) return fail(c, MP_ERR_ARG, "mp_anchor_set: col[%d] = %d is not ascending inside [0, %d)", j, col[j], L);
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    free_anchor(c);
    // host side of the upload: codes, the 12-mer of every position, the table of positions, the inverse column map
    std::vector<uint8_t> code((size_t)n);
    for (int32_t j = 0; j < n; j++) code[(size_t)j] = (uint8_t)base_code(codes[j]);
    std::vector<uint32_t> kmer((size_t)n, kEmpty);
    for (int32_t j = 0; j + kWord <= n; j++) {
        uint32_t w = 0;
        bool ok = true;
        for (int x = 0; x < kWord; x++) { ok = ok && code[(size_t)(j + x)] < 4; w = (w << 2) | (code[(size_t)(j + x)] & 3u); }
        if (ok) kmer[(size_t)j] = w;
    }
    int log2_slots = 4;
    while ((1 << log2_slots) < 2 * n) log2_slots++;
    const int32_t slots = 1 << log2_slots;
    std::vector<int32_t> table((size_t)slots, -1);
    for (int32_t j = 0; j < n; j++) {
        if (kmer[(size_t)j] == kEmpty) continue;
        uint32_t s = word_hash(kmer[(size_t)j], log2_slots);
        while (table[s] >= 0) s = (s + 1) & (uint32_t)(slots - 1);
        table[s] = j;
    }
    std::vector<int32_t> colinv((size_t)L, -1);
    for (int32_t j = 0; j < n; j++) colinv[(size_t)col[j]] = j;
    c->an_n = n; c->an_L = L; c->an_slots = slots;
    int rc;
    if ((rc = dev_alloc(c, &c->an_code, (size_t)n)) || (rc = dev_alloc(c, &c->an_kmer, (size_t)n)) || (rc = dev_alloc(c, &c->an_table, (size_t)slots)) ||
        (rc = dev_alloc(c, &c->an_col, (size_t)n)) || (rc = dev_alloc(c, &c->an_colinv, (size_t)L))) { free_anchor(c); return rc; }
    hipError_t e = hipMemcpyAsync(c->an_code, code.data(), (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->an_kmer, kmer.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->an_table, table.data(), sizeof(int32_t) * (size_t)slots, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->an_col, col, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->an_colinv, colinv.data(), sizeof(int32_t) * (size_t)L, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);          // (the host arrays leave scope)
    if (e != hipSuccess) { free_anchor(c); return fail(c, MP_ERR_DEVICE, "mp_anchor_set: %s", hipGetErrorString(e)); }
    for (int i = 0; i < 6; i++) c->an_par[i] = par[i];
    return MP_OK;
}

int mp_anchor_align(mp_ctx *c, int32_t nq, const uint8_t *bytes, const int64_t *off, int32_t want_ops, uint8_t *rows_out, int32_t *meta_out,
                    uint8_t *ops_out, const int64_t *ops_off) {
    if (!c) return MP_ERR_ARG;
    if (c->an_n == 0) return fail(c, MP_ERR_ARG, "mp_anchor_align: no anchor (mp_anchor_set first)");
    if (nq < 0 || (nq && (!bytes || !off || !rows_out || !meta_out)) || (nq && want_ops && (!ops_out || !ops_off)))
        return fail(c, MP_ERR_ARG, "mp_anchor_align: bad arguments");
    const auto t0 = std::chrono::steady_clock::now();
    for (double &x : c->an_ms) x = 0;
    for (int64_t &x : c->an_counts) x = 0;
    if (nq == 0) return MP_OK;
    const int n = c->an_n, L = c->an_L, W = c->an_par[4], B = 2 * W + 1;
    const int R = B <= 64 ? 1 : B <= 128 ? 2 : B <= 256 ? 4 : 8, Bpad = 64 * R;
    for (int32_t q = 0; q < nq; q++) {
        const int64_t m = off[q + 1] - off[q];
        if (m < 1 || m > MP_ANCHOR_MAX_LEN) return fail(c, MP_ERR_ARG, "mp_anchor_align: query %d has %lld bases (1..%d)", q, (long long)m, MP_ANCHOR_MAX_LEN);
        if (want_ops && ops_off[q + 1] - ops_off[q] < m + n)
            return fail(c, MP_ERR_ARG, "mp_anchor_align: the ops slot of query %d holds %lld bytes, %lld needed", q, (long long)(ops_off[q + 1] - ops_off[q]), (long long)(m + n));
    }
    HIPCK(c, hipSetDevice(c->dev));
    // batches: the traceback words of a batch stay within a quarter of the free device memory
    size_t free_b = 0, total_b = 0;
    HIPCK(c, hipMemGetInfo(&free_b, &total_b));
    const size_t tb_budget = std::max<size_t>(free_b / 4 / sizeof(uint32_t), (size_t)1 << 22);      // words
    long long cap_q = 1 << 20;
    if (const char *s = getenv("MP_ANCHOR_BATCH")) { const long long v = atoll(s); if (v > 0) cap_q = v; }
    auto tb_words = [&](int32_t q) { return (size_t)((off[q + 1] - off[q] + 7) / 8) * (size_t)Bpad; };
    std::vector<int32_t> bstart{0};
    {
        size_t w = 0;
        for (int32_t q = 0; q < nq; q++) {
            const size_t wq = tb_words(q);
            if (q > bstart.back() && (w + wq > tb_budget || q - bstart.back() >= cap_q)) { bstart.push_back(q); w = 0; }
            w += wq;
        }
        bstart.push_back(nq);
    }
    size_t max_q = 0, max_bytes = 0, max_tb = 0, max_ops = 0;
    int max_m = 0;
    for (size_t b = 0; b + 1 < bstart.size(); b++) {
        const int32_t q0 = bstart[b], q1 = bstart[b + 1];
        size_t w = 0;
        for (int32_t q = q0; q < q1; q++) { w += tb_words(q); max_m = std::max(max_m, (int)(off[q + 1] - off[q])); }
        max_q = std::max(max_q, (size_t)(q1 - q0));
        max_bytes = std::max(max_bytes, (size_t)(off[q1] - off[q0]));
        max_tb = std::max(max_tb, w);
        if (want_ops) max_ops = std::max(max_ops, (size_t)(ops_off[q1] - ops_off[q0]));
    }
    uint8_t *d_bytes = nullptr, *d_arow = nullptr, *d_rows = nullptr, *d_ops = nullptr;
    int64_t *d_off = nullptr, *d_tboff = nullptr, *d_opsoff = nullptr;
    int32_t *d_d0 = nullptr, *d_end = nullptr, *d_meta = nullptr;
    uint32_t *d_tb = nullptr;
    auto cleanup = [&]() {
        dev_free(c, &d_bytes, max_bytes); dev_free(c, &d_arow, max_q * n); dev_free(c, &d_rows, max_q * L); dev_free(c, &d_ops, max_ops);
        dev_free(c, &d_off, max_q + 1); dev_free(c, &d_tboff, max_q + 1); dev_free(c, &d_opsoff, max_q + 1); dev_free(c, &d_d0, max_q);
        dev_free(c, &d_end, 2 * max_q); dev_free(c, &d_meta, max_q * MP_ANCHOR_META); dev_free(c, &d_tb, max_tb);
    };
    int rc;
    if ((rc = dev_alloc(c, &d_bytes, max_bytes)) || (rc = dev_alloc(c, &d_arow, max_q * n)) || (rc = dev_alloc(c, &d_rows, max_q * L)) ||
        (rc = dev_alloc(c, &d_ops, max_ops)) || (rc = dev_alloc(c, &d_off, max_q + 1)) || (rc = dev_alloc(c, &d_tboff, max_q + 1)) ||
        (rc = dev_alloc(c, &d_opsoff, max_q + 1)) || (rc = dev_alloc(c, &d_d0, max_q)) || (rc = dev_alloc(c, &d_end, 2 * max_q)) ||
        (rc = dev_alloc(c, &d_meta, max_q * MP_ANCHOR_META)) || (rc = dev_alloc(c, &d_tb, max_tb))) { cleanup(); return rc; }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
    auto finish = [&](int code) { (void)hipStreamSynchronize(c->stream); for (auto &x : ev) if (x) (void)hipEventDestroy(x); cleanup(); return code; };
    if (e != hipSuccess) return finish(fail(c, MP_ERR_DEVICE, "mp_anchor_align: %s", hipGetErrorString(e)));
    // LDS of a launch: the vote histogram of the longest query; the anchor and the queries of a workgroup's waves
    const size_t vote_lds = ((size_t)(max_m + n) / 2 + 1) * sizeof(uint32_t);
    if (vote_lds > 65536) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(anchor_vote_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)vote_lds);
        if (e != hipSuccess) return finish(fail(c, MP_ERR_DEVICE, "mp_anchor_align: %s", hipGetErrorString(e)));
    }
    const int npad = (n + 15) & ~15, mstride = (max_m + 15) & ~15;
    const int wpb = npad + 4 * mstride <= 32768 ? 4 : 1;          // four queries share one anchor copy while five workgroups still fit a CU
    const size_t dp_lds = (size_t)npad + (size_t)wpb * mstride;   // (at most 64 KiB: 32768 + 32768)
    int log2_slots = 0;
    while ((1 << log2_slots) < c->an_slots) log2_slots++;
    std::vector<int64_t> h_off, h_tboff, h_opsoff;
    long long cells = 0;
    for (size_t b = 0; b + 1 < bstart.size(); b++) {
        const int32_t q0 = bstart[b], q1 = bstart[b + 1], nb = q1 - q0;
        h_off.assign((size_t)nb + 1, 0); h_tboff.assign((size_t)nb + 1, 0); h_opsoff.assign((size_t)nb + 1, 0);
        for (int32_t q = 0; q <= nb; q++) {
            h_off[(size_t)q] = off[q0 + q] - off[q0];
            if (want_ops) h_opsoff[(size_t)q] = ops_off[q0 + q] - ops_off[q0];
            if (q < nb) { h_tboff[(size_t)q + 1] = h_tboff[(size_t)q] + (int64_t)tb_words(q0 + q); cells += (long long)(off[q0 + q + 1] - off[q0 + q]) * B; }
        }
        e = hipMemcpyAsync(d_bytes, bytes + off[q0], (size_t)(off[q1] - off[q0]), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_off, h_off.data(), sizeof(int64_t) * ((size_t)nb + 1), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_tboff, h_tboff.data(), sizeof(int64_t) * ((size_t)nb + 1), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && want_ops) e = hipMemcpyAsync(d_opsoff, h_opsoff.data(), sizeof(int64_t) * ((size_t)nb + 1), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipEventRecord(ev[0], c->stream);
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(anchor_vote_kernel, dim3((unsigned)nb), dim3(64), vote_lds, c->stream, (const uint8_t *)d_bytes, (const int64_t *)d_off, n,
                           (const uint32_t *)c->an_kmer, (const int32_t *)c->an_table, log2_slots, d_d0);
        if ((e = hipGetLastError()) != hipSuccess) break;
        if ((e = hipEventRecord(ev[1], c->stream)) != hipSuccess) break;
        const dim3 grid((unsigned)((nb + wpb - 1) / wpb)), block((unsigned)(64 * wpb));
#define MP_ANCHOR_DP(RR)                                                                                                                         \
        hipLaunchKernelGGL((anchor_dp_kernel<RR>), grid, block, dp_lds, c->stream, (const uint8_t *)d_bytes, (const int64_t *)d_off, (int)nb,        \
                           (const int32_t *)d_d0, (const uint8_t *)c->an_code, n, W, (int)c->an_par[0], (int)c->an_par[1],                          \
                           (int)(c->an_par[2] + c->an_par[3]), (int)c->an_par[3], mstride, d_tb, (const int64_t *)d_tboff, d_end)
        if (R == 1) MP_ANCHOR_DP(1); else if (R == 2) MP_ANCHOR_DP(2); else if (R == 4) MP_ANCHOR_DP(4); else MP_ANCHOR_DP(8);
#undef MP_ANCHOR_DP
        if ((e = hipGetLastError()) != hipSuccess) break;
        if ((e = hipEventRecord(ev[2], c->stream)) != hipSuccess) break;
        hipLaunchKernelGGL(anchor_trace_kernel, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, c->stream, (const uint8_t *)d_bytes, (const int64_t *)d_off,
                           (int)nb, (const int32_t *)d_d0, (const uint8_t *)c->an_code, (const int32_t *)c->an_col, n, W, R, (int)c->an_par[5],
                           (const uint32_t *)d_tb, (const int64_t *)d_tboff, (const int32_t *)d_end, d_arow, d_meta, want_ops ? d_ops : (uint8_t *)nullptr,
                           (const int64_t *)d_opsoff);
        if ((e = hipGetLastError()) != hipSuccess) break;
        const long long total = (long long)nb * L;
        hipLaunchKernelGGL(anchor_emit_kernel, dim3((unsigned)((total + 4095) / 4096)), dim3(256), 0, c->stream, (const uint8_t *)d_arow,
                           (const int32_t *)d_meta, (const int32_t *)c->an_colinv, n, L, total, d_rows);
        if ((e = hipGetLastError()) != hipSuccess) break;
        if ((e = hipEventRecord(ev[3], c->stream)) != hipSuccess) break;
        if ((e = hipEventSynchronize(ev[3])) != hipSuccess) break;
        const auto t1 = std::chrono::steady_clock::now();
        e = hipMemcpyAsync(rows_out + (size_t)q0 * L, d_rows, (size_t)total, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(meta_out + (size_t)q0 * MP_ANCHOR_META, d_meta, sizeof(int32_t) * (size_t)nb * MP_ANCHOR_META, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && want_ops) e = hipMemcpyAsync(ops_out + ops_off[q0], d_ops, (size_t)(ops_off[q1] - ops_off[q0]), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) break;
        c->an_ms[3] += ms_since(t1);
        for (int i = 0; i < 3; i++) {
            float ms = 0;
            if ((e = hipEventElapsedTime(&ms, ev[i], ev[i + 1])) != hipSuccess) break;
            c->an_ms[i] += ms;
        }
        if (e != hipSuccess) break;
    }
    if (e != hipSuccess) return finish(fail(c, MP_ERR_DEVICE, "mp_anchor_align: %s", hipGetErrorString(e)));
    for (int32_t q = 0; q < nq; q++)
        if (meta_out[(size_t)q * MP_ANCHOR_META + 7] & 4) return finish(fail(c, MP_ERR_DEVICE, "mp_anchor_align: the traceback of query %d left its band", q));
    c->an_counts[0] = (int64_t)bstart.size() - 1;
    c->an_counts[1] = cells;
    c->an_counts[2] = (int64_t)(max_tb * sizeof(uint32_t));
    rc = finish(MP_OK);
    c->an_ms[4] = ms_since(t0);
    return rc;
}

int mp_anchor_stats(mp_ctx *c, double *ms, int64_t *counts) {
    if (!c) return MP_ERR_ARG;
    for (int i = 0; i < 5; i++) if (ms) ms[i] = c->an_ms[i];
    for (int i = 0; i < 3; i++) if (counts) counts[i] = c->an_counts[i];
    return MP_OK;
}

}  // extern "C"
