// scan.hip — part of libmprime_hip.so: hand-written HIP (gfx950 / MI355X, wave64) behind the C ABI of include/mprime.h.
// (8) k-mismatch primer-site scan over unaligned sequences (mp_kmm_scan) — the GPU replacement of the bowtie2 + samtools
// mapping step of scripts/primer_coverage_validation_by_BWT_V9.py (BWT:264-300) and of its MD:Z filter (BWT:241-262).
//
// Shape: a workgroup owns one segment of one sequence.  It packs the segment once into LDS — 2 bits per base plus a
// "never matches" bit for everything outside ACGT — and every thread then slides over its start positions: the 32-base
// window at a position is two LDS words and a funnel shift (a second 32-base window for patterns of 33..64 bases: the
// two-word kernel), and one pattern costs an XOR, a fold of the two bits of each base, a mask, a popcount and two compares
// per word.  The pattern table (code word, length mask, trailing-run mask per strand) is
// wave-uniform and arrives through scalar loads.  HBM traffic is the text once (1 byte per base); the work is integer VALU:
// ~10 wave-instructions per (64 positions, pattern).
#include "common.hpp"
#include "kmm.hpp"
#include "../../include/mprime_offtarget.h"

using namespace mp;

namespace {

// pack the characters of the store into words (one thread per word; once per mp_seq_load)
__global__ __launch_bounds__(kBlock) void seq_pack_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ row_off,
                                                          const int64_t *__restrict__ woff, int n_rows, unsigned long long *__restrict__ code,
                                                          unsigned long long *__restrict__ flag) {
    const int row = blockIdx.x;
    if (row >= n_rows) return;
    const uint8_t *s = bytes + row_off[row];
    const long long len = row_off[row + 1] - row_off[row], nw = woff[row + 1] - woff[row];
    for (long long w = threadIdx.x; w < nw; w += kBlock) {
        unsigned long long b = 0, f = 0;
        for (int j = 0; j < 32; j++) {
            const long long p = w * 32 + j;
            unsigned long long c = 0, bad = 1, low = 0;
            if (p < len) {
                uint8_t ch = s[p];
                if (ch >= 'a' && ch <= 'z') { ch -= 32; low = 1; }
                if (ch == 'A') { c = 0; bad = 0; }
                else if (ch == 'C') { c = 1; bad = 0; }
                else if (ch == 'G') { c = 2; bad = 0; }
                else if (ch == 'T') { c = 3; bad = 0; }
            }
            b |= c << (2 * j);
            f |= (bad | (low << 1)) << (2 * j);
        }
        code[woff[row] + w] = b;
        flag[woff[row] + w] = f;
    }
}

// the scan itself on device text X (the bytes of this call, or the resident store); max_gap >= 0: the gapped rule of mprime_offtarget.h
// with the penalty ceiling `budget`, else `budget` mismatches (kmm_tables)
int kmm_scan_device(mp_ctx *c, const KmmText &X, const int64_t *roff_host, int32_t n_rows, int32_t n_pat, const uint8_t *pat_codes,
                    const int32_t *pat_off, int32_t budget, int32_t max_gap, int32_t term, int64_t cap, int32_t *hits, int64_t *n_hits) {
    int rc;
    if ((rc = kmm_check_patterns(c, n_pat, pat_codes, pat_off))) return rc;
    std::vector<int32_t> all((size_t)n_pat);                              // one budget: every pattern in one table
    std::iota(all.begin(), all.end(), 0);
    const KmmTable T = kmm_budget(kmm_table(all, pat_codes, pat_off, nullptr, term), budget, max_gap);
    KmmBlocks B(c);
    if ((rc = B.build(roff_host, n_rows))) return rc;
    if (B.size() == 0) return MP_OK;
    DevBuf<int32_t> d_hits(c);
    DevBuf<uint8_t> d_pats(c);
    DevBuf<unsigned long long> d_n(c);
    if ((rc = d_hits.alloc((size_t)std::max<int64_t>(cap, 1) * 4)) || (rc = d_pats.alloc(T.bytes.size())) || (rc = d_n.alloc(1))) return rc;
    HIPCK_WAIT(c, B.upload());
    HIPCK_WAIT(c, d_pats.upload(T.bytes.data(), T.bytes.size()));
    HIPCK_WAIT(c, d_n.zero());
    HIPCK_WAIT(c, (kmm_launch<kKmmBytes | kKmmGaps>(c, X, B, T, d_pats.p, term, KmmAppend{(long long)cap, d_hits.p, d_n.p})));
    unsigned long long n = 0;
    HIPCK_WAIT(c, hipMemcpyAsync(&n, d_n.p, sizeof n, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));              // (the block list and the table may go now)
    const size_t got = cap ? (size_t)std::min<unsigned long long>(n, (unsigned long long)cap) : 0;
    if (got) {
        HIPCK_WAIT(c, hipMemcpyAsync(hits, d_hits.p, sizeof(int32_t) * 4 * got, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
    }
    *n_hits = (int64_t)n;
    return MP_OK;
}

}  // namespace

namespace mp {
void free_seq(mp_ctx *c) {
    dev_free(c, &c->sq_bytes, c->sq_total + 16); dev_free(c, &c->sq_roff, (size_t)c->sq_n + 1);
    dev_free(c, &c->sq_code, c->sq_words); dev_free(c, &c->sq_flag, c->sq_words); dev_free(c, &c->sq_woff, (size_t)c->sq_n + 1);
    c->sq_n = 0; c->sq_total = c->sq_words = 0;
    c->sq_roff_host.clear();
    dev_free(c, &c->ot_out, (size_t)c->ot_n * 6);      // products of mp_offtarget_resident belong to the store they came from
    c->ot_n = 0;
    c->ot_key.clear();
    c->otc_out.clear();
    c->otc_key.clear();
    free_setscreen(c, true);                           // a set screen belongs to the store it was opened on
}
}  // namespace mp

extern "C" {

int mp_seq_load(mp_ctx *c, const uint8_t *bytes, const int64_t *row_off, int32_t n_rows) {
    if (!c) return MP_ERR_ARG;
    if (n_rows < 0 || (n_rows && (!bytes || !row_off))) return fail(c, MP_ERR_ARG, "mp_seq_load: bad arguments");
    HIPCK(c, hipSetDevice(c->dev));
    free_seq(c);
    if (n_rows == 0) return MP_OK;
    std::vector<int64_t> roff((size_t)n_rows + 1), woff((size_t)n_rows + 1);
    woff[0] = 0;
    for (int32_t r = 0; r <= n_rows; r++) roff[(size_t)r] = row_off[r] - row_off[0];
    for (int32_t r = 0; r < n_rows; r++) {
        const int64_t len = roff[(size_t)r + 1] - roff[(size_t)r];
        if (len < 0 || len > 0x7fffffffLL) return fail(c, MP_ERR_ARG, "sequence %d has bad length", r);
        woff[(size_t)r + 1] = woff[(size_t)r] + (len + 31) / 32;
    }
    const size_t total = (size_t)roff[(size_t)n_rows], words = (size_t)woff[(size_t)n_rows];
    int rc;
    c->sq_n = n_rows; c->sq_total = total; c->sq_words = words;
    if ((rc = dev_alloc(c, &c->sq_bytes, total + 16)) || (rc = dev_alloc(c, &c->sq_roff, (size_t)n_rows + 1)) || (rc = dev_alloc(c, &c->sq_code, words)) ||
        (rc = dev_alloc(c, &c->sq_flag, words)) || (rc = dev_alloc(c, &c->sq_woff, (size_t)n_rows + 1))) { free_seq(c); return rc; }
    hipError_t e = hipSuccess;
    if (total) e = hipMemcpyAsync(c->sq_bytes, bytes + row_off[0], total, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->sq_roff, roff.data(), sizeof(int64_t) * roff.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->sq_woff, woff.data(), sizeof(int64_t) * woff.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(seq_pack_kernel, dim3((unsigned)n_rows), dim3(kBlock), 0, c->stream, (const uint8_t *)c->sq_bytes, (const int64_t *)c->sq_roff,
                           (const int64_t *)c->sq_woff, (int)n_rows, c->sq_code, c->sq_flag);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);            // (the host vectors above leave scope)
    if (e != hipSuccess) { free_seq(c); return fail(c, MP_ERR_DEVICE, "mp_seq_load: %s", hipGetErrorString(e)); }
    c->sq_roff_host = std::move(roff);
    return MP_OK;
}

int mp_seq_free(mp_ctx *c) {
    if (!c) return MP_ERR_ARG;
    HIPCK(c, hipSetDevice(c->dev));
    free_seq(c);
    return MP_OK;
}

int mp_seq_info(mp_ctx *c, int32_t *n_rows, int64_t *n_bases, int64_t *device_bytes) {
    if (!c) return MP_ERR_ARG;
    if (n_rows) *n_rows = c->sq_n;
    if (n_bases) *n_bases = (int64_t)c->sq_total;
    if (device_bytes) *device_bytes = c->sq_n ? (int64_t)(c->sq_total + 16 + 16 * c->sq_words + 16 * ((size_t)c->sq_n + 1)) : 0;
    return MP_OK;
}

int mp_kmm_scan(mp_ctx *c, const uint8_t *bytes, const int64_t *row_off, int32_t n_rows, int32_t n_pat, const uint8_t *pat_codes,
                const int32_t *pat_off, int32_t max_mm, int32_t term, int64_t cap, int32_t *hits, int64_t *n_hits) {
    if (!c) return MP_ERR_ARG;
    if (n_rows < 0 || n_pat < 0 || !n_hits || cap < 0 || (cap && !hits) || (n_rows && (!bytes || !row_off)) ||
        (n_pat && (!pat_codes || !pat_off)) || max_mm < 0 || term < 0)
        return fail(c, MP_ERR_ARG, "mp_kmm_scan: bad arguments");
    HIPCK(c, hipSetDevice(c->dev));
    *n_hits = 0;
    if (n_rows == 0 || n_pat == 0) return MP_OK;
    const size_t total = (size_t)(row_off[n_rows] - row_off[0]);
    std::vector<int64_t> roff((size_t)n_rows + 1);
    for (int32_t r = 0; r <= n_rows; r++) roff[(size_t)r] = row_off[r] - row_off[0];
    DevBuf<uint8_t> d_bytes(c);
    DevBuf<int64_t> d_roff(c);
    int rc;
    if ((rc = d_bytes.alloc(total + 16)) || (rc = d_roff.alloc((size_t)n_rows + 1))) return rc;
    HIPCK_WAIT(c, d_bytes.upload(bytes + row_off[0], total));
    HIPCK_WAIT(c, d_roff.upload(roff.data(), roff.size()));
    rc = kmm_scan_device(c, KmmText{d_bytes.p, d_roff.p, nullptr, nullptr, nullptr}, roff.data(), n_rows, n_pat, pat_codes, pat_off, max_mm, -1, term,
                         cap, hits, n_hits);
    (void)hipStreamSynchronize(c->stream);                  // (roff leaves scope)
    return rc;
}

int mp_kmm_scan_resident(mp_ctx *c, int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off, int32_t max_mm, int32_t term, int64_t cap,
                         int32_t *hits, int64_t *n_hits) {
    if (!c) return MP_ERR_ARG;
    if (n_pat < 0 || !n_hits || cap < 0 || (cap && !hits) || (n_pat && (!pat_codes || !pat_off)) || max_mm < 0 || term < 0)
        return fail(c, MP_ERR_ARG, "mp_kmm_scan_resident: bad arguments");
    HIPCK(c, hipSetDevice(c->dev));
    *n_hits = 0;
    if (c->sq_n == 0 || n_pat == 0) return MP_OK;
    return kmm_scan_device(c, kmm_store(c), c->sq_roff_host.data(), c->sq_n, n_pat, pat_codes, pat_off, max_mm, -1, term, cap, hits, n_hits);
}

int mp_kmm_gap_scan_resident(mp_ctx *c, int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off, int32_t max_pen, int32_t max_gap,
                             int32_t term, int64_t cap, int32_t *hits, int64_t *n_hits) {
    if (!c) return MP_ERR_ARG;
    if (n_pat < 0 || !n_hits || cap < 0 || (cap && !hits) || (n_pat && (!pat_codes || !pat_off)) || max_pen < 0 || term < 0)
        return fail(c, MP_ERR_ARG, "mp_kmm_gap_scan_resident: bad arguments");
    if (max_gap < 0 || max_gap > MP_KMM_MAX_GAP) return fail(c, MP_ERR_ARG, "mp_kmm_gap_scan_resident: max_gap %d (0..%d)", max_gap, MP_KMM_MAX_GAP);
    HIPCK(c, hipSetDevice(c->dev));
    *n_hits = 0;
    if (c->sq_n == 0 || n_pat == 0) return MP_OK;
    // (no gap fits under the ceiling, 5 + 3 g > max_penalty, or none is asked for: the ungapped kernel, exactly)
    return kmm_scan_device(c, kmm_store(c), c->sq_roff_host.data(), c->sq_n, n_pat, pat_codes, pat_off, max_pen, max_gap, term, cap, hits, n_hits);
}

}  // extern "C"
