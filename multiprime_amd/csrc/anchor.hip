// anchor.hip — anchored alignment (include/mprime_anchor.h): every query is placed on the anchor of a seed alignment by a banded
// affine-gap (Gotoh) alignment around a voted seed diagonal.  The vote, sweep and traceback kernels are those of anchorcore.hpp (the sweep's
// rule itself: bandsweep.hpp; the 12-mer of a position, here for the anchor's table: seedword.hpp); here:
//   anchor_emit_kernel   expands anchor space to the seed's L columns: 16 row bytes per lane, one 128-bit store each
#include "anchorcore.hpp"

namespace mp {

namespace {

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
    for (int32_t j = 0; j + kWord <= n; j++) kmer[(size_t)j] = seed_word_codes(code.data() + j);
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
    const int R = lane_diagonals(W), Bpad = 64 * R;
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
    uint8_t *d_turn = nullptr;                 // both strands: 1 per query of the batch that anchor_orient_kernel turned
    const bool both = c->an_both != 0;
    auto cleanup = [&]() {
        dev_free(c, &d_bytes, max_bytes); dev_free(c, &d_arow, max_q * n); dev_free(c, &d_rows, max_q * L); dev_free(c, &d_ops, max_ops);
        dev_free(c, &d_off, max_q + 1); dev_free(c, &d_tboff, max_q + 1); dev_free(c, &d_opsoff, max_q + 1); dev_free(c, &d_d0, max_q);
        dev_free(c, &d_end, 2 * max_q); dev_free(c, &d_meta, max_q * MP_ANCHOR_META); dev_free(c, &d_tb, max_tb);
        dev_free(c, &d_turn, max_q);
    };
    int rc;
    if ((rc = dev_alloc(c, &d_bytes, max_bytes)) || (rc = dev_alloc(c, &d_arow, max_q * n)) || (rc = dev_alloc(c, &d_rows, max_q * L)) ||
        (rc = dev_alloc(c, &d_ops, max_ops)) || (rc = dev_alloc(c, &d_off, max_q + 1)) || (rc = dev_alloc(c, &d_tboff, max_q + 1)) ||
        (rc = dev_alloc(c, &d_opsoff, max_q + 1)) || (rc = dev_alloc(c, &d_d0, max_q)) || (rc = dev_alloc(c, &d_end, 2 * max_q)) ||
        (rc = dev_alloc(c, &d_meta, max_q * MP_ANCHOR_META)) || (rc = dev_alloc(c, &d_tb, max_tb)) ||
        (both && (rc = dev_alloc(c, &d_turn, max_q)))) { cleanup(); return rc; }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
    auto finish = [&](int code) { (void)hipStreamSynchronize(c->stream); for (auto &x : ev) if (x) (void)hipEventDestroy(x); cleanup(); return code; };
    if (e != hipSuccess) return finish(fail(c, MP_ERR_DEVICE, "mp_anchor_align: %s", hipGetErrorString(e)));
    // LDS of a launch: the vote histogram of the longest query; the anchor and the queries of a workgroup's waves
    const size_t vote_lds = ((size_t)(max_m + n) / 2 + 1) * sizeof(uint32_t);
    if (vote_lds > 65536) {
        e = hipFuncSetAttribute(both ? reinterpret_cast<const void *>(anchor_orient_kernel<false>) : reinterpret_cast<const void *>(anchor_vote_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)vote_lds);
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
        if (both)          // the batch's device copy of the turned queries becomes rc(q): the sweep, the traceback and the emit read it as it is
            hipLaunchKernelGGL(anchor_orient_kernel<false>, dim3((unsigned)nb), dim3(64), vote_lds, c->stream, d_bytes, (const int64_t *)d_off, n,
                               (const uint32_t *)c->an_kmer, (const int32_t *)c->an_table, log2_slots, d_d0, d_turn);
        else
            hipLaunchKernelGGL(anchor_vote_kernel, dim3((unsigned)nb), dim3(64), vote_lds, c->stream, (const uint8_t *)d_bytes, (const int64_t *)d_off, n,
                               (const uint32_t *)c->an_kmer, (const int32_t *)c->an_table, log2_slots, d_d0);
        if ((e = hipGetLastError()) != hipSuccess) break;
        if ((e = hipEventRecord(ev[1], c->stream)) != hipSuccess) break;
        const dim3 grid((unsigned)((nb + wpb - 1) / wpb)), block((unsigned)(64 * wpb));
        for_lane_diagonals(W, [&](auto r) {
            hipLaunchKernelGGL((anchor_dp_kernel<decltype(r)::value, false>), grid, block, dp_lds, c->stream, (const uint8_t *)d_bytes, (const int64_t *)d_off,
                               (int)nb, (const int32_t *)d_d0, (const uint8_t *)c->an_code, n, W, (int)c->an_par[0], (int)c->an_par[1],
                               (int)(c->an_par[2] + c->an_par[3]), (int)c->an_par[3], mstride, d_tb, (const int64_t *)d_tboff, d_end,
                               (const int32_t *)nullptr, 0LL);
        });
        if ((e = hipGetLastError()) != hipSuccess) break;
        if ((e = hipEventRecord(ev[2], c->stream)) != hipSuccess) break;
        hipLaunchKernelGGL((anchor_trace_kernel<false, false>), dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, c->stream, (const uint8_t *)d_bytes, (const int64_t *)d_off,
                           (int)nb, (const int32_t *)d_d0, (const uint8_t *)c->an_code, (const int32_t *)c->an_col, n, W, R, (int)c->an_par[5],
                           (const uint32_t *)d_tb, (const int64_t *)d_tboff, (const int32_t *)d_end, d_arow, d_meta, want_ops ? d_ops : (uint8_t *)nullptr,
                           (const int64_t *)d_opsoff, (const int32_t *)nullptr, 0LL, (uint16_t *)nullptr, (uint16_t *)nullptr, 0);
        if ((e = hipGetLastError()) != hipSuccess) break;
        if (both) {
            hipLaunchKernelGGL(anchor_mark_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, c->stream, d_meta, (const uint8_t *)d_turn, (int)nb);
            if ((e = hipGetLastError()) != hipSuccess) break;
        }
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

int mp_anchor_strands(mp_ctx *c, int32_t both) {
    if (!c) return MP_ERR_ARG;
    c->an_both = both != 0;
    return MP_OK;
}

int mp_anchor_stats(mp_ctx *c, double *ms, int64_t *counts) {
    if (!c) return MP_ERR_ARG;
    for (int i = 0; i < 5; i++) if (ms) ms[i] = c->an_ms[i];
    for (int i = 0; i < 3; i++) if (counts) counts[i] = c->an_counts[i];
    return MP_OK;
}

}  // extern "C"
