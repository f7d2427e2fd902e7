// star.hip — the star alignment (include/mprime_star.h): one round aligns every resident record to an anchor with the vote, sweep and
// traceback kernels of anchorcore.hpp (the sweep's rule and the launch over its R forms: bandsweep.hpp) and turns the N pairwise paths into
// one alignment that keeps every inserted base.  New here:
//   path store            the traceback (kStore) notes per record and slot the inserted run's length and first query base: two
//                         uint16 [N][S] planes, S = n + 1 rounded up to 8 so that a record's slots start on 16 bytes
//   star_flag_kernel      band escalation: the records of a batch whose path touched the band (or found none) as an ascending list with
//                         the offsets of their traceback words at the wider band — one workgroup, a block scan of (count, words)
//   star_clear_kernel     the listed records' run lengths back to zero before their traceback is walked again
//   star_profile_kernel   ins[j] = max over the placed records of run_len[.][j]: a lane reads eight slots (16 bytes) of a record, lanes
//                         side by side in j, 256 records to a workgroup, one atomicMax per non-zero slot and workgroup
//   star_scan_kernel      acol[j] = j + sum(ins[g], g <= j) and L' — n + 1 <= 32768 slots: one workgroup, 32 slots to a thread
//   star_map_kernel       column -> anchor position j, or ~slot
//   star_write_kernel     rows [N][L']: 16 output bytes per lane and one 128-bit store, the tail of the buffer by bytes
//   star_count_kernel     per column A, C, G, T, other letter, gap over the placed rows: a lane reads 16 bytes of a row and keeps packed
//                         16-bit counters over up to 256 rows, a workgroup adds them up in LDS, one global atomicAdd per non-zero
//                         (column, class) and 1024 rows
// Nothing per cell or per base leaves the device between rounds: a round hands back the meta records, ins, L' and (on request) the counts.
#include "anchorcore.hpp"
#include "../../include/mprime_star.h"

namespace mp {

namespace {

constexpr int kFlagThreads = 1024;
constexpr int kProfileRows = 256;              // records per workgroup of star_profile_kernel
constexpr int kCountCols = 1024, kCountRows = 1024;   // tile of star_count_kernel: 64 lanes x 16 columns, 4 waves x up to 256 rows

inline long long tb_words_of(long long m, int Bpad) { return ((m + 7) / 8) * (long long)Bpad; }

__global__ __launch_bounds__(kFlagThreads) void star_flag_kernel(const int32_t *__restrict__ meta, const int64_t *__restrict__ off, int q0, int nb,
                                                                  int bpad, int w_next, int32_t *__restrict__ list, int64_t *__restrict__ tboff,
                                                                  int32_t *__restrict__ wfin, int64_t *__restrict__ out) {
    __shared__ long long s_cnt[kFlagThreads], s_words[kFlagThreads];
    const int tid = threadIdx.x, per = (nb + kFlagThreads - 1) / kFlagThreads;
    const int lo = min(nb, tid * per), hi = min(nb, lo + per);
    long long cnt = 0, words = 0;
    for (int x = lo; x < hi; x++) {
        const int q = q0 + x;
        if (meta[(size_t)q * MP_ANCHOR_META + 7] & 2) { cnt++; words += ((off[q + 1] - off[q] + 7) / 8) * (long long)bpad; }
    }
    s_cnt[tid] = cnt;
    s_words[tid] = words;
    __syncthreads();
    for (int d = 1; d < kFlagThreads; d <<= 1) {
        const long long a = tid >= d ? s_cnt[tid - d] : 0, b = tid >= d ? s_words[tid - d] : 0;
        __syncthreads();
        s_cnt[tid] += a;
        s_words[tid] += b;
        __syncthreads();
    }
    long long at = s_cnt[tid] - cnt, w = s_words[tid] - words;
    for (int x = lo; x < hi; x++) {
        const int q = q0 + x;
        if (meta[(size_t)q * MP_ANCHOR_META + 7] & 2) {
            list[at] = q;
            tboff[at] = w;
            wfin[q] = w_next;
            at++;
            w += ((off[q + 1] - off[q] + 7) / 8) * (long long)bpad;
        }
    }
    if (tid == kFlagThreads - 1) {
        out[0] = s_cnt[tid];
        out[1] = s_words[tid];
        tboff[s_cnt[tid]] = s_words[tid];
    }
}

__global__ __launch_bounds__(256) void star_clear_kernel(const int32_t *__restrict__ list, uint16_t *__restrict__ run_len, int S) {
    uint32_t *row = reinterpret_cast<uint32_t *>(run_len + (size_t)list[blockIdx.x] * S);      // (S is a multiple of 8)
    for (int x = threadIdx.x; x < S / 2; x += 256) row[x] = 0;
}

__global__ __launch_bounds__(256) void star_profile_kernel(const uint16_t *__restrict__ run_len, const int32_t *__restrict__ meta, int N, int S,
                                                            int32_t *__restrict__ ins) {
    const int g = blockIdx.y * 256 + threadIdx.x;          // slots 8 g .. 8 g + 7
    if (8 * g >= S) return;
    const int r0 = blockIdx.x * kProfileRows, r1 = min(N, r0 + kProfileRows);
    uint32_t mx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = r0; r < r1; r++) {
        if (meta[(size_t)r * MP_ANCHOR_META + 7] & 1) continue;          // not placed (uniform over the workgroup)
        const uint4 v = *reinterpret_cast<const uint4 *>(run_len + (size_t)r * S + 8 * g);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            mx[2 * k] = max(mx[2 * k], w[k] & 0xFFFFu);
            mx[2 * k + 1] = max(mx[2 * k + 1], w[k] >> 16);
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (mx[k]) atomicMax(&ins[8 * g + k], (int32_t)mx[k]);
}

// one workgroup: thread t owns slots [t * per, t * per + per)
__global__ __launch_bounds__(1024) void star_scan_kernel(const int32_t *__restrict__ ins, int n, int32_t *__restrict__ acol, int32_t *__restrict__ width) {
    __shared__ int s_sum[1024];
    const int tid = threadIdx.x, slots = n + 1, per = (slots + 1023) / 1024;
    const int lo = min(slots, tid * per), hi = min(slots, lo + per);
    int sum = 0;
    for (int j = lo; j < hi; j++) sum += ins[j];
    s_sum[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int a = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += a;
        __syncthreads();
    }
    int run = s_sum[tid] - sum;
    for (int j = lo; j < hi; j++) {
        run += ins[j];
        acol[j] = j + run;                     // (acol[n] = n + sum of all = L': slot n ends where the row ends)
    }
    if (tid == 1023) *width = n + s_sum[1023];
}

__global__ __launch_bounds__(256) void star_map_kernel(const int32_t *__restrict__ ins, const int32_t *__restrict__ acol, int n, int L,
                                                        int32_t *__restrict__ colmap) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j > n) return;
    const int a = acol[j], k = ins[j];
    if (j < n && a < L) colmap[a] = j;
    for (int o = 0; o < k; o++)
        if (a - k + o >= 0 && a - k + o < L) colmap[a - k + o] = ~j;
}

// rows [N][L] as one run of bytes: lane g writes bytes 16 g .. 16 g + 15 (the buffer starts on a hipMalloc boundary)
__global__ __launch_bounds__(256) void star_write_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ off,
                                                          const int32_t *__restrict__ meta, const uint8_t *__restrict__ arow,
                                                          const uint16_t *__restrict__ run_len, const uint16_t *__restrict__ q_start, int S,
                                                          const int32_t *__restrict__ ins, const int32_t *__restrict__ acol,
                                                          const int32_t *__restrict__ colmap, int n, int L, long long total,
                                                          uint8_t *__restrict__ rows) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x, b0 = g * 16;
    if (b0 >= total) return;
    long long q = b0 / L;
    int c = (int)(b0 - q * L);
    const int32_t *mt = meta + q * MP_ANCHOR_META;
    bool placed = !(mt[7] & 1);
    int jf = mt[8], jl = mt[9];
    const uint8_t *qb = bytes + off[q];
    uint32_t w[4] = {0, 0, 0, 0};
    const int cnt = (int)min(16LL, total - b0);
#pragma unroll
    for (int x = 0; x < 16; x++) {
        uint8_t ch = '-';
        if (x < cnt) {
            if (placed) {
                const int code = colmap[c];
                if (code >= 0) {
                    if (code >= jf && code <= jl) ch = arow[(size_t)q * n + code];
                } else {
                    const int s = ~code, len = run_len[(size_t)q * S + s];
                    if (len) {
                        const int o = c - (acol[s] - ins[s]), qs = q_start[(size_t)q * S + s];
                        if (qs == 0) {         // the run before the first aligned base: right-justified
                            const int k = o - (ins[s] - len);
                            if (k >= 0) ch = upper_letter(qb[k]);
                        } else if (o < len) ch = upper_letter(qb[qs + o]);
                    }
                }
            }
            if (++c == L) {
                c = 0;
                q++;
                if (x + 1 < cnt) {
                    mt = meta + q * MP_ANCHOR_META;
                    placed = !(mt[7] & 1);
                    jf = mt[8];
                    jl = mt[9];
                    qb = bytes + off[q];
                }
            }
        }
        w[x >> 2] |= (uint32_t)ch << (8 * (x & 3));
    }
    if (cnt == 16) *reinterpret_cast<uint4 *>(rows + b0) = make_uint4(w[0], w[1], w[2], w[3]);
    else
        for (int x = 0; x < cnt; x++) rows[b0 + x] = (uint8_t)(w[x >> 2] >> (8 * (x & 3)));
}

__global__ __launch_bounds__(256) void star_count_kernel(const uint8_t *__restrict__ rows, const int32_t *__restrict__ meta, int N, int L,
                                                          int32_t *__restrict__ counts) {
    __shared__ int s_cnt[kCountCols * MP_STAR_COUNTS];
    const int tid = threadIdx.x, cg = tid & 63, rl = tid >> 6;
    for (int e = tid; e < kCountCols * MP_STAR_COUNTS; e += 256) s_cnt[e] = 0;
    __syncthreads();
    const int c0 = blockIdx.y * kCountCols + cg * 16, nv = min(16, L - c0);
    const int r0 = blockIdx.x * kCountRows, r1 = min(N, r0 + kCountRows);
    if (nv > 0) {
        uint32_t ac[16], gt[16], og[16];       // two 16-bit counters each (at most 256 rows per lane): A | C, G | T, other | gap
#pragma unroll
        for (int x = 0; x < 16; x++) ac[x] = gt[x] = og[x] = 0;
        for (int r = r0 + rl; r < r1; r += 4) {
            if (meta[(size_t)r * MP_ANCHOR_META + 7] & 1) continue;
            const uint8_t *p = rows + (size_t)r * L + c0;
            uint8_t b[16];
            if (nv == 16) __builtin_memcpy(b, p, 16);
            else
                for (int x = 0; x < 16; x++) b[x] = x < nv ? p[x] : (uint8_t)0;
#pragma unroll
            for (int x = 0; x < 16; x++) {
                const uint8_t ch = b[x];
                const uint32_t isA = ch == 'A', isC = ch == 'C', isG = ch == 'G', isT = ch == 'T', isGap = ch == '-';
                ac[x] += isA | (isC << 16);
                gt[x] += isG | (isT << 16);
                og[x] += (uint32_t)(x < nv && !(isA | isC | isG | isT | isGap)) | (isGap << 16);
            }
        }
#pragma unroll
        for (int x = 0; x < 16; x++) {
            if (x >= nv) continue;
            int *s = s_cnt + (cg * 16 + x) * MP_STAR_COUNTS;
            const uint32_t v[6] = {ac[x] & 0xFFFFu, ac[x] >> 16, gt[x] & 0xFFFFu, gt[x] >> 16, og[x] & 0xFFFFu, og[x] >> 16};
#pragma unroll
            for (int k = 0; k < 6; k++)
                if (v[k]) atomicAdd(&s[k], (int)v[k]);
        }
    }
    __syncthreads();
    for (int e = tid; e < kCountCols * MP_STAR_COUNTS; e += 256) {
        const int col = blockIdx.y * kCountCols + e / MP_STAR_COUNTS;
        if (col < L && s_cnt[e]) atomicAdd(&counts[(size_t)col * MP_STAR_COUNTS + e % MP_STAR_COUNTS], s_cnt[e]);
    }
}

// the arrays of one round (kept after it for mp_star_rows / mp_star_counts)
void free_round(mp_ctx *c) {
    const size_t N = (size_t)c->st_n, S = (size_t)c->st_stride;
    dev_free(c, &c->st_d0, N); dev_free(c, &c->st_end, 2 * N); dev_free(c, &c->st_meta, N * MP_ANCHOR_META); dev_free(c, &c->st_wfin, N);
    dev_free(c, &c->st_arow, N * (size_t)c->st_an); dev_free(c, &c->st_runlen, N * S); dev_free(c, &c->st_qstart, N * S);
    dev_free(c, &c->st_ins, S); dev_free(c, &c->st_acol, S); dev_free(c, &c->st_colmap, (size_t)c->st_width);
    dev_free(c, &c->st_rows, N * (size_t)c->st_width); dev_free(c, &c->st_colcnt, (size_t)c->st_width * MP_STAR_COUNTS);
    c->st_an = c->st_stride = c->st_width = 0;
}

}  // namespace

void free_star(mp_ctx *c) {
    free_round(c);
    dev_free(c, &c->st_bytes, c->st_total);
    dev_free(c, &c->st_off, (size_t)c->st_n + 1);
    dev_free(c, &c->st_parity, (size_t)c->st_n);
    c->st_n = 0;
    c->st_total = 0;
    c->st_off_host.clear();
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_star_load(mp_ctx *c, int32_t n, const uint8_t *bytes, const int64_t *off) {
    if (!c) return MP_ERR_ARG;
    if (n < 1 || !bytes || !off) return fail(c, MP_ERR_ARG, "mp_star_load: bad arguments (at least one record)");
    for (int32_t q = 0; q < n; q++) {
        const int64_t m = off[q + 1] - off[q];
        if (m < 1 || m > MP_ANCHOR_MAX_LEN) return fail(c, MP_ERR_ARG, "mp_star_load: record %d has %lld bases (1..%d)", q, (long long)m, MP_ANCHOR_MAX_LEN);
    }
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    free_star(c);
    c->st_n = n;
    c->st_total = (size_t)(off[n] - off[0]);
    c->st_off_host.resize((size_t)n + 1);
    for (int32_t q = 0; q <= n; q++) c->st_off_host[(size_t)q] = off[q] - off[0];
    int rc;
    if ((rc = dev_alloc(c, &c->st_bytes, c->st_total)) || (rc = dev_alloc(c, &c->st_off, (size_t)n + 1)) ||
        (rc = dev_alloc(c, &c->st_parity, (size_t)n))) { free_star(c); return rc; }
    hipError_t e = hipMemcpyAsync(c->st_bytes, bytes + off[0], c->st_total, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->st_parity, 0, (size_t)n, c->stream);        // every record is held as given
    if (e == hipSuccess) e = hipMemcpyAsync(c->st_off, c->st_off_host.data(), sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { free_star(c); return fail(c, MP_ERR_DEVICE, "mp_star_load: %s", hipGetErrorString(e)); }
    return MP_OK;
}

int mp_star_round(mp_ctx *c, const uint8_t *anchor, int32_t n, const mp_anchor_params *p, int32_t *meta_out, int32_t *ins_out, int32_t *width_out) {
    if (!c) return MP_ERR_ARG;
    if (c->st_n == 0) return fail(c, MP_ERR_ARG, "mp_star_round: no records (mp_star_load first)");
    if (!anchor || !p || !meta_out || !ins_out || !width_out) return fail(c, MP_ERR_ARG, "mp_star_round: null argument");
    if (p->band < 1) return fail(c, MP_ERR_ARG, "mp_star_round: band %d (1..%d: a band of 0 never grows)", p->band, MP_ANCHOR_MAX_BAND);
    const auto t0 = std::chrono::steady_clock::now();
    for (double &x : c->st_ms) x = 0;
    for (int64_t &x : c->st_counts) x = 0;
    {
        std::vector<int32_t> ident((size_t)std::max(n, 0));
        std::iota(ident.begin(), ident.end(), 0);
        const int rc = mp_anchor_set(c, anchor, n, ident.data(), n, p);      // every check of the anchor and the parameters; the 12-mer table
        if (rc) return rc;
    }
    HIPCK(c, hipSetDevice(c->dev));
    free_round(c);
    const int N = c->st_n, W0 = p->band, S = (n + 1 + 7) & ~7;
    const std::vector<int64_t> &off = c->st_off_host;
    // the per-round store, sized for all records
    const size_t store_bytes = (size_t)N * S * 2 * sizeof(uint16_t) + (size_t)N * n;
    size_t free_b = 0, total_b = 0;
    HIPCK(c, hipMemGetInfo(&free_b, &total_b));
    if (store_bytes > free_b + c->pool_bytes)
        return fail(c, MP_ERR_CAPACITY, "mp_star_round: the path store of %d records x %d slots takes %zu bytes, %zu are free", N, n + 1, store_bytes, free_b);
    c->st_an = n; c->st_stride = S;
    int rc;
    if ((rc = dev_alloc(c, &c->st_d0, (size_t)N)) || (rc = dev_alloc(c, &c->st_end, 2 * (size_t)N)) || (rc = dev_alloc(c, &c->st_meta, (size_t)N * MP_ANCHOR_META)) ||
        (rc = dev_alloc(c, &c->st_wfin, (size_t)N)) || (rc = dev_alloc(c, &c->st_arow, (size_t)N * n)) || (rc = dev_alloc(c, &c->st_runlen, (size_t)N * S)) ||
        (rc = dev_alloc(c, &c->st_qstart, (size_t)N * S)) || (rc = dev_alloc(c, &c->st_ins, (size_t)S)) || (rc = dev_alloc(c, &c->st_acol, (size_t)S))) {
        free_round(c);
        return rc;
    }
    // batches: the traceback words of a batch stay within a quarter of the free device memory
    HIPCK(c, hipMemGetInfo(&free_b, &total_b));
    const size_t tb_budget = std::max<size_t>(free_b / 4 / sizeof(uint32_t), (size_t)1 << 22);      // words
    long long cap_q = 1 << 20;
    if (const char *s = getenv("MP_STAR_BATCH")) { const long long v = atoll(s); if (v > 0) cap_q = std::min(v, cap_q); }
    const int R0 = lane_diagonals(W0);
    std::vector<int32_t> bstart{0};
    size_t tb_cap = 0, max_q = 0;
    int max_m = 0;
    {
        size_t w = 0;
        for (int32_t q = 0; q < N; q++) {
            const long long m = off[(size_t)q + 1] - off[(size_t)q];
            const size_t wq = (size_t)tb_words_of(m, 64 * R0);
            if (q > bstart.back() && (w + wq > tb_budget || q - bstart.back() >= cap_q)) { bstart.push_back(q); w = 0; }
            w += wq;
            tb_cap = std::max(tb_cap, std::max(w, (size_t)tb_words_of(m, 512)));          // a batch at W, or one record at the widest band
            max_m = std::max(max_m, (int)m);
        }
        bstart.push_back(N);
        for (size_t b = 0; b + 1 < bstart.size(); b++) max_q = std::max(max_q, (size_t)(bstart[b + 1] - bstart[b]));
    }
    uint32_t *d_tb = nullptr;
    int64_t *d_tboff = nullptr, *d_flag = nullptr;
    int32_t *d_list = nullptr;
    std::vector<hipEvent_t> evs;
    std::vector<int> tags;
    auto finish = [&](int code) {
        (void)hipStreamSynchronize(c->stream);
        for (auto &x : evs) (void)hipEventDestroy(x);
        dev_free(c, &d_tb, tb_cap); dev_free(c, &d_tboff, max_q + 1); dev_free(c, &d_flag, (size_t)2); dev_free(c, &d_list, max_q);
        if (code != MP_OK) free_round(c);
        return code;
    };
    if ((rc = dev_alloc(c, &d_tb, tb_cap)) || (rc = dev_alloc(c, &d_tboff, max_q + 1)) || (rc = dev_alloc(c, &d_flag, (size_t)2)) ||
        (rc = dev_alloc(c, &d_list, max_q))) return finish(rc);
    hipError_t e = hipSuccess;
    // mark(tag): the device time since the previous mark belongs to stage `tag` (-1: to nobody — the host was in between)
    auto mark = [&](int tag) {
        hipEvent_t ev = nullptr;
        if (e == hipSuccess) e = hipEventCreate(&ev);
        if (e == hipSuccess) { evs.push_back(ev); tags.push_back(tag); e = hipEventRecord(ev, c->stream); }
        return e == hipSuccess;
    };
    auto launched = [&]() { if (e == hipSuccess) e = hipGetLastError(); return e == hipSuccess; };
    auto dev_fail = [&]() { return finish(fail(c, MP_ERR_DEVICE, "mp_star_round: %s", hipGetErrorString(e))); };
    const bool both = c->an_both != 0;
    const size_t vote_lds = ((size_t)(max_m + n) / 2 + 1) * sizeof(uint32_t);
    if (vote_lds > 65536) {
        e = hipFuncSetAttribute(both ? reinterpret_cast<const void *>(anchor_orient_kernel<true>) : reinterpret_cast<const void *>(anchor_vote_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)vote_lds);
        if (e != hipSuccess) return dev_fail();
    }
    const int npad = (n + 15) & ~15, mstride = (max_m + 15) & ~15;
    const int wpb = npad + 4 * mstride <= 32768 ? 4 : 1;
    const size_t dp_lds = (size_t)npad + (size_t)wpb * mstride;
    int log2_slots = 0;
    while ((1 << log2_slots) < c->an_slots) log2_slots++;
    const int oe = (int)(p->gap_open + p->gap_extend), ext = (int)p->gap_extend, permille = (int)p->min_identity_permille;
    const int32_t *no_list = nullptr;
    // sweep + traceback of `items` work items at band W: the records q0 .. q0 + items (list == null) or list[0 .. items)
    auto align = [&](int W, int items, int q0, const int32_t *list, const int64_t *tboff, long long tb_base) {
        const int R = lane_diagonals(W);
        const dim3 grid((unsigned)((items + wpb - 1) / wpb)), block((unsigned)(64 * wpb));
        const int64_t *offp = c->st_off + q0;
        const int32_t *d0p = c->st_d0 + q0;
        int32_t *endp = c->st_end + 2 * (size_t)q0;
        auto sweep = [&](auto r, auto listed) {
            hipLaunchKernelGGL((anchor_dp_kernel<decltype(r)::value, decltype(listed)::value>), grid, block, dp_lds, c->stream, (const uint8_t *)c->st_bytes,
                               offp, items, d0p, (const uint8_t *)c->an_code, n, W, (int)p->match, (int)p->mismatch, oe, ext, mstride, d_tb, tboff, endp,
                               list, tb_base);
        };
        for_lane_diagonals(W, [&](auto r) { if (list) sweep(r, std::true_type{}); else sweep(r, std::false_type{}); });
        if (!launched() || !mark(1)) return false;
#define MP_STAR_TRACE(LL)                                                                                                                         \
        hipLaunchKernelGGL((anchor_trace_kernel<LL, true>), dim3((unsigned)((items + 63) / 64)), dim3(64), 0, c->stream, (const uint8_t *)c->st_bytes,  \
                           offp, items, d0p, (const uint8_t *)c->an_code, (const int32_t *)c->an_col, n, W, R, permille, (const uint32_t *)d_tb, tboff,    \
                           (const int32_t *)endp, c->st_arow + (size_t)q0 * n, c->st_meta + (size_t)q0 * MP_ANCHOR_META, (uint8_t *)nullptr,              \
                           (const int64_t *)nullptr, list, tb_base, c->st_runlen + (size_t)q0 * S, c->st_qstart + (size_t)q0 * S, S)
        if (list) MP_STAR_TRACE(true); else MP_STAR_TRACE(false);
#undef MP_STAR_TRACE
        return launched() && mark(2);
    };
    long long cells = 0, again = 0;
    e = hipMemsetAsync(c->st_runlen, 0, sizeof(uint16_t) * (size_t)N * S, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->st_ins, 0, sizeof(int32_t) * (size_t)S, c->stream);
    if (e != hipSuccess) return dev_fail();
    {
        const FillSeg seg{c->st_wfin, sizeof(int32_t) * (size_t)N, (uint32_t)W0};
        if ((rc = fill_segments(c, &seg, 1))) return finish(rc);
    }
    if (!mark(-1)) return dev_fail();
    if (both)              // a turned record stays turned in the resident bytes; st_parity is its orientation against the loaded record
        hipLaunchKernelGGL(anchor_orient_kernel<true>, dim3((unsigned)N), dim3(64), vote_lds, c->stream, c->st_bytes, (const int64_t *)c->st_off, n,
                           (const uint32_t *)c->an_kmer, (const int32_t *)c->an_table, log2_slots, c->st_d0, c->st_parity);
    else
        hipLaunchKernelGGL(anchor_vote_kernel, dim3((unsigned)N), dim3(64), vote_lds, c->stream, (const uint8_t *)c->st_bytes, (const int64_t *)c->st_off, n,
                           (const uint32_t *)c->an_kmer, (const int32_t *)c->an_table, log2_slots, c->st_d0);
    if (!launched() || !mark(0)) return dev_fail();
    std::vector<int64_t> h_tboff;
    for (size_t b = 0; b + 1 < bstart.size(); b++) {
        const int32_t q0 = bstart[b], nb = bstart[b + 1] - q0;
        h_tboff.assign((size_t)nb + 1, 0);
        for (int32_t q = 0; q < nb; q++) {
            const long long m = off[(size_t)q0 + q + 1] - off[(size_t)q0 + q];
            h_tboff[(size_t)q + 1] = h_tboff[(size_t)q] + tb_words_of(m, 64 * R0);
            cells += m * (2 * W0 + 1);
        }
        e = hipMemcpyAsync(d_tboff, h_tboff.data(), sizeof(int64_t) * ((size_t)nb + 1), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess || !mark(-1)) return dev_fail();
        if (!align(W0, nb, q0, no_list, d_tboff, 0)) return dev_fail();
        // band escalation: the flagged records of this batch again at twice the band, until none is left or the band is the widest
        for (int W = W0; W < MP_ANCHOR_MAX_BAND;) {
            W = std::min(2 * W, MP_ANCHOR_MAX_BAND);
            const int Bpad = 64 * lane_diagonals(W);
            hipLaunchKernelGGL(star_flag_kernel, dim3(1), dim3(kFlagThreads), 0, c->stream, (const int32_t *)c->st_meta, (const int64_t *)c->st_off, (int)q0,
                               (int)nb, Bpad, W, d_list, d_tboff, c->st_wfin, d_flag);
            if (!launched() || !mark(2)) return dev_fail();
            int64_t flag[2] = {0, 0};
            e = hipMemcpyAsync(flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return dev_fail();
            const int64_t n_list = flag[0];
            if (n_list == 0) break;
            if (n_list < 0 || n_list > nb) return finish(fail(c, MP_ERR_DEVICE, "mp_star_round: %lld of %d records flagged", (long long)n_list, nb));
            again += n_list;
            h_tboff.assign((size_t)n_list + 1, 0);
            e = hipMemcpyAsync(h_tboff.data(), d_tboff, sizeof(int64_t) * ((size_t)n_list + 1), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess || !mark(-1)) return dev_fail();
            hipLaunchKernelGGL(star_clear_kernel, dim3((unsigned)n_list), dim3(256), 0, c->stream, (const int32_t *)d_list, c->st_runlen, S);
            if (!launched() || !mark(2)) return dev_fail();
            // chunks of the list whose words fit the buffer (one record at the widest band always does)
            for (int64_t s0 = 0; s0 < n_list;) {
                int64_t s1 = s0 + 1;
                while (s1 < n_list && s1 - s0 < cap_q && (size_t)(h_tboff[(size_t)s1 + 1] - h_tboff[(size_t)s0]) <= tb_cap) s1++;
                if ((size_t)(h_tboff[(size_t)s1] - h_tboff[(size_t)s0]) > tb_cap)
                    return finish(fail(c, MP_ERR_DEVICE, "mp_star_round: a record's traceback words exceed the buffer"));
                cells += (h_tboff[(size_t)s1] - h_tboff[(size_t)s0]) / Bpad * 8 * (2 * W + 1);       // (rows rounded up to eight)
                if (!align(W, (int)(s1 - s0), 0, d_list + s0, d_tboff + s0, (long long)h_tboff[(size_t)s0])) return dev_fail();
                s0 = s1;
            }
        }
    }
    // the insertion profile, the columns, the rows, the counts
    if (!mark(-1)) return dev_fail();
    if (both) {            // (after the last traceback: an escalated record's meta record was written again)
        hipLaunchKernelGGL(anchor_mark_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, c->st_meta, (const uint8_t *)c->st_parity, N);
        if (!launched()) return dev_fail();
    }
    hipLaunchKernelGGL(star_profile_kernel, dim3((unsigned)((N + kProfileRows - 1) / kProfileRows), (unsigned)((S / 8 + 255) / 256)), dim3(256), 0, c->stream,
                       (const uint16_t *)c->st_runlen, (const int32_t *)c->st_meta, N, S, c->st_ins);
    if (!launched()) return dev_fail();
    hipLaunchKernelGGL(star_scan_kernel, dim3(1), dim3(1024), 0, c->stream, (const int32_t *)c->st_ins, (int)n, c->st_acol, (int32_t *)d_flag);
    if (!launched() || !mark(3)) return dev_fail();
    int32_t L = 0;
    e = hipMemcpyAsync(&L, d_flag, sizeof L, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return dev_fail();
    if (L < n) return finish(fail(c, MP_ERR_DEVICE, "mp_star_round: width %d for %d anchor positions", L, n));
    if ((L + kCountCols - 1) / kCountCols > 65535)
        return finish(fail(c, MP_ERR_CAPACITY, "mp_star_round: %d columns (at most %d)", L, 65535 * kCountCols));
    c->st_width = L;
    if ((rc = dev_alloc(c, &c->st_colmap, (size_t)L)) || (rc = dev_alloc(c, &c->st_rows, (size_t)N * L)) ||
        (rc = dev_alloc(c, &c->st_colcnt, (size_t)L * MP_STAR_COUNTS))) return finish(rc);
    e = hipMemsetAsync(c->st_colcnt, 0, sizeof(int32_t) * (size_t)L * MP_STAR_COUNTS, c->stream);
    if (e != hipSuccess || !mark(-1)) return dev_fail();
    hipLaunchKernelGGL(star_map_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, c->stream, (const int32_t *)c->st_ins, (const int32_t *)c->st_acol,
                       (int)n, (int)L, c->st_colmap);
    if (!launched() || !mark(3)) return dev_fail();
    const long long total = (long long)N * L;
    hipLaunchKernelGGL(star_write_kernel, dim3((unsigned)((total + 4095) / 4096)), dim3(256), 0, c->stream, (const uint8_t *)c->st_bytes, (const int64_t *)c->st_off,
                       (const int32_t *)c->st_meta, (const uint8_t *)c->st_arow, (const uint16_t *)c->st_runlen, (const uint16_t *)c->st_qstart, S,
                       (const int32_t *)c->st_ins, (const int32_t *)c->st_acol, (const int32_t *)c->st_colmap, (int)n, (int)L, total, c->st_rows);
    if (!launched() || !mark(4)) return dev_fail();
    hipLaunchKernelGGL(star_count_kernel, dim3((unsigned)((N + kCountRows - 1) / kCountRows), (unsigned)((L + kCountCols - 1) / kCountCols)), dim3(256), 0,
                       c->stream, (const uint8_t *)c->st_rows, (const int32_t *)c->st_meta, N, (int)L, c->st_colcnt);
    if (!launched() || !mark(5)) return dev_fail();
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return dev_fail();
    // read-back: per record and per slot only
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<int32_t> h_meta((size_t)N * MP_ANCHOR_META), h_wfin((size_t)N);
    e = hipMemcpyAsync(h_meta.data(), c->st_meta, sizeof(int32_t) * h_meta.size(), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_wfin.data(), c->st_wfin, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ins_out, c->st_ins, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return dev_fail();
    int64_t placed = 0;
    for (int32_t q = 0; q < N; q++) {
        const int32_t *mt = &h_meta[(size_t)q * MP_ANCHOR_META];
        if (mt[7] & 4) return finish(fail(c, MP_ERR_DEVICE, "mp_star_round: the traceback of record %d left its band", q));
        std::copy(mt, mt + MP_ANCHOR_META, meta_out + (size_t)q * MP_STAR_META);
        meta_out[(size_t)q * MP_STAR_META + MP_ANCHOR_META] = h_wfin[(size_t)q];
        placed += !(mt[7] & 1);
    }
    *width_out = L;
    c->st_ms[6] = ms_since(t1);
    for (size_t i = 1; i < evs.size(); i++) {
        if (tags[i] < 0) continue;
        float ms = 0;
        if ((e = hipEventElapsedTime(&ms, evs[i - 1], evs[i])) != hipSuccess) return dev_fail();
        c->st_ms[tags[i]] += ms;
    }
    c->st_counts[0] = (int64_t)bstart.size() - 1;
    c->st_counts[1] = cells;
    c->st_counts[2] = again;
    c->st_counts[3] = (int64_t)(tb_cap * sizeof(uint32_t));
    c->st_counts[4] = (int64_t)store_bytes;
    c->st_counts[5] = placed;
    rc = finish(MP_OK);
    c->st_ms[7] = ms_since(t0);
    return rc;
}

int mp_star_rows(mp_ctx *c, uint8_t *rows_out) {
    if (!c) return MP_ERR_ARG;
    if (!c->st_rows || !rows_out) return fail(c, MP_ERR_ARG, "mp_star_rows: no round (mp_star_round first)");
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipMemcpyAsync(rows_out, c->st_rows, (size_t)c->st_n * (size_t)c->st_width, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return MP_OK;
}

int mp_star_counts(mp_ctx *c, int32_t *counts_out) {
    if (!c) return MP_ERR_ARG;
    if (!c->st_colcnt || !counts_out) return fail(c, MP_ERR_ARG, "mp_star_counts: no round (mp_star_round first)");
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipMemcpyAsync(counts_out, c->st_colcnt, sizeof(int32_t) * (size_t)c->st_width * MP_STAR_COUNTS, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return MP_OK;
}

int mp_star_stats(mp_ctx *c, double *ms, int64_t *counts) {
    if (!c) return MP_ERR_ARG;
    for (int i = 0; i < 8; i++) if (ms) ms[i] = c->st_ms[i];
    for (int i = 0; i < 6; i++) if (counts) counts[i] = c->st_counts[i];
    return MP_OK;
}

int mp_star_free(mp_ctx *c) {
    if (!c) return MP_ERR_ARG;
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    free_star(c);
    return MP_OK;
}

}  // extern "C"
