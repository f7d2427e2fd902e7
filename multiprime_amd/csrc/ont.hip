// ont.hip — read ends against expanded primers (include/mprime_ont.h): the Ratcliff/Obershelp match count M of difflib for every
// (piece, key) pair and, per piece, the key of the highest rank q[T][M], the first one among equals.  One kernel:
//   ont_assign_kernel<W> block (x, y): 256 pieces (one per lane, four position masks of type W in registers) against key split y.  Keys
//                       are wave-uniform (five 64-bit words each: masks A, C, G, T and length | base counts, scalar loads).  A pair walks
//                       its pending ranges from an LDS stack (one column per lane); a range's longest common substring is the longest
//                       run of ones over its diagonals, diagonal d = OR_c piece[c] & shift(key[c], d).  A lane keeps its own best over
//                       the split's keys and leaves it with one 64-bit atomicMax.
// W = uint32_t when no piece of the launch and no key has more than 32 bytes, else uint64_t.  Integers only; the rank table comes from the caller.
#include "common.hpp"
#include "ontcore.hpp"

namespace mp {

namespace {

constexpr int kOntBlock = 256;
constexpr int kOntKeyWords = 5;                // masks A, C, G, T; info = length | count A << 8 | C << 16 | G << 24 | T << 32
constexpr int kQCols = MP_ONT_Q_COLS;
constexpr int64_t kOntChunk = (int64_t)1 << 22;   // pieces per launch

template <typename W>
__global__ __launch_bounds__(kOntBlock) void ont_assign_kernel(const W *__restrict__ pm, const uint32_t *__restrict__ plen, int n_pieces,
                                                               const uint64_t *__restrict__ keys, int n_keys, int keys_per_block,
                                                               const int32_t *__restrict__ q, int prune, unsigned long long *__restrict__ out) {
    __shared__ uint32_t stack[ont_stack_entries<W>() * kOntBlock];
    const int p = (int)(blockIdx.x * kOntBlock + threadIdx.x);
    if (p >= n_pieces) return;                 // (no barrier below)
    W pa[4];
    for (int c = 0; c < 4; c++) pa[c] = pm[(size_t)c * (size_t)n_pieces + (size_t)p];
    const int la = (int)plen[p];
    int cnt[4];
    for (int c = 0; c < 4; c++) cnt[c] = ont_popc(pa[c]);
    uint32_t *stk = stack + threadIdx.x;
    const int k0 = (int)blockIdx.y * keys_per_block, k1 = min(n_keys, k0 + keys_per_block);
    int best_q = -1, best_key = 0, best_m = 0;
    for (int k = k0; k < k1; k++) {
        const uint64_t *kp = keys + (size_t)k * kOntKeyWords;
        const W kb[4] = {(W)kp[0], (W)kp[1], (W)kp[2], (W)kp[3]};
        const uint64_t info = kp[4];
        const int lb = (int)(info & 0xFF);
        const int32_t *qrow = q + (la + lb) * kQCols;
        if (prune) {
            const int ub = min(cnt[0], (int)((info >> 8) & 0xFF)) + min(cnt[1], (int)((info >> 16) & 0xFF)) + min(cnt[2], (int)((info >> 24) & 0xFF)) +
                           min(cnt[3], (int)((info >> 32) & 0xFF));
            if (qrow[ub] <= best_q) continue;  // q does not decrease along M, and an equal q at a later index does not win
        }
        const int M = ont_matches<W>(pa, la, kb, lb, stk, kOntBlock);
        const int qq = qrow[M];
        if (qq > best_q) { best_q = qq; best_key = k; best_m = M; }
    }
    if (best_q >= 0)
        atomicMax(out + p, ((unsigned long long)best_q << 40) | ((unsigned long long)(0xFFFFFFFFu - (uint32_t)best_key) << 8) | (unsigned long long)best_m);
}

int ont_dev(mp_ctx *c, hipError_t e, const char *who, const char *what) {
    return e == hipSuccess ? MP_OK : fail(c, MP_ERR_DEVICE, "%s: %s: %s", who, what, hipGetErrorString(e));
}

}  // namespace

void free_ont(mp_ctx *c) {
    dev_free(c, &c->ont_keys, (size_t)c->ont_n * kOntKeyWords);
    dev_free(c, &c->ont_q, (size_t)MP_ONT_Q_ROWS * MP_ONT_Q_COLS);
    c->ont_n = 0;
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_ont_set_keys(mp_ctx *c, int32_t n_keys, const uint8_t *bytes, const int64_t *off) {
    static const char *who = "mp_ont_set_keys";
    if (!c) return MP_ERR_ARG;
    if (!bytes || !off) return fail(c, MP_ERR_ARG, "%s: null argument", who);
    if (n_keys < 1 || n_keys > MP_ONT_MAX_KEYS) return fail(c, MP_ERR_ARG, "%s: %d keys (1..%d)", who, n_keys, MP_ONT_MAX_KEYS);
    std::vector<uint64_t> h((size_t)n_keys * kOntKeyWords);
    int max_len = 0;
    for (int32_t i = 0; i < n_keys; i++) {
        const int64_t len = off[i + 1] - off[i];
        if (len < 0 || len > MP_ONT_MAX_LEN) return fail(c, MP_ERR_ARG, "%s: key %d has %lld bytes (0..%d)", who, i, (long long)len, MP_ONT_MAX_LEN);
        const uint8_t *b = bytes + off[i];
        for (int64_t x = 0; x < len; x++)
            if (ont_code(b[x]) > 3) return fail(c, MP_ERR_ARG, "%s: key %d holds byte 0x%02X at %lld (upper-case A, C, G, T only)", who, i, b[x], (long long)x);
        uint64_t *k = h.data() + (size_t)i * kOntKeyWords;
        ont_masks(b, (int)len, k);
        k[4] = (uint64_t)len;
        max_len = std::max(max_len, (int)len);
        for (int cd = 0; cd < 4; cd++) k[4] |= (uint64_t)__builtin_popcountll(k[cd]) << (8 + 8 * cd);
    }
    HIPCK(c, hipSetDevice(c->dev));
    HIPCK(c, hipStreamSynchronize(c->stream));
    free_ont(c);
    c->ont_ms = 0;
    c->ont_counts[0] = c->ont_counts[1] = 0;
    c->ont_n = n_keys;
    c->ont_max_len = max_len;
    int rc;
    if ((rc = dev_alloc(c, &c->ont_keys, h.size())) == MP_OK && (rc = dev_alloc(c, &c->ont_q, (size_t)MP_ONT_Q_ROWS * MP_ONT_Q_COLS)) == MP_OK)
        rc = ont_dev(c, hipMemcpy(c->ont_keys, h.data(), sizeof(uint64_t) * h.size(), hipMemcpyHostToDevice), who, "copy");
    if (rc) { free_ont(c); return rc; }
    c->ont_counts[0] = n_keys;
    return MP_OK;
}

int mp_ont_assign(mp_ctx *c, int64_t n_pieces, const uint8_t *bytes, const int64_t *off, const int32_t *q, int32_t *key, int32_t *m) {
    static const char *who = "mp_ont_assign";
    if (!c) return MP_ERR_ARG;
    if (c->ont_n == 0) return fail(c, MP_ERR_ARG, "%s: no keys (mp_ont_set_keys first)", who);
    if (n_pieces < 0 || !q || (n_pieces && (!bytes || !off || !key || !m))) return fail(c, MP_ERR_ARG, "%s: bad arguments", who);
    for (int t = 0; t < MP_ONT_Q_ROWS; t++)
        for (int x = 0; x < MP_ONT_Q_COLS; x++) {
            const int32_t v = q[t * MP_ONT_Q_COLS + x];
            if (v < 0 || v > 65535 || (x && v < q[t * MP_ONT_Q_COLS + x - 1]))
                return fail(c, MP_ERR_ARG, "%s: q[%d][%d] = %d (0..65535, not decreasing along M)", who, t, x, v);
        }
    for (int64_t p = 0; p < n_pieces; p++) {
        const int64_t len = off[p + 1] - off[p];
        if (len < 0 || len > MP_ONT_MAX_LEN) return fail(c, MP_ERR_ARG, "%s: piece %lld has %lld bytes (0..%d)", who, (long long)p, (long long)len, MP_ONT_MAX_LEN);
    }
    if (n_pieces == 0) return MP_OK;
    const char *e = getenv("MP_ONT_PRUNE");
    const int prune = e && atoi(e) == 0 ? 0 : 1;
    e = getenv("MP_ONT_KEYS_PER_BLOCK");
    const int forced = e ? atoi(e) : 0;
    e = getenv("MP_ONT_WORD");
    const bool wide_only = e && atoi(e) == 64;
    HIPCK(c, hipSetDevice(c->dev));
    const size_t cap = (size_t)std::min<int64_t>(n_pieces, kOntChunk);
    uint64_t *d_pm = nullptr;
    uint32_t *d_len = nullptr;
    unsigned long long *d_out = nullptr;
    std::vector<uint64_t> h_pm(cap * 4);
    std::vector<uint32_t> h_len(cap);
    std::vector<unsigned long long> h_out(cap);
    int rc;
    if ((rc = dev_alloc(c, &d_pm, cap * 4)) == MP_OK && (rc = dev_alloc(c, &d_len, cap)) == MP_OK && (rc = dev_alloc(c, &d_out, cap)) == MP_OK)
        rc = ont_dev(c, hipMemcpyAsync(c->ont_q, q, sizeof(int32_t) * MP_ONT_Q_ROWS * MP_ONT_Q_COLS, hipMemcpyHostToDevice, c->stream), who, "copy");
    for (int64_t p0 = 0; p0 < n_pieces && rc == MP_OK; p0 += kOntChunk) {
        const int nb = (int)std::min<int64_t>(kOntChunk, n_pieces - p0);
        int longest = 0;
        for (int x = 0; x < nb; x++) longest = std::max(longest, (int)(off[p0 + x + 1] - off[p0 + x]));
        // 32-bit masks when no piece of the launch and no key has more than 32 bytes (MP_ONT_WORD=64: always 64-bit masks)
        const bool narrow = !wide_only && longest <= 32 && c->ont_max_len <= 32;
        uint32_t *h_pm32 = reinterpret_cast<uint32_t *>(h_pm.data());
        for (int x = 0; x < nb; x++) {
            uint64_t pm[4];
            const int len = (int)(off[p0 + x + 1] - off[p0 + x]);
            ont_masks(bytes + off[p0 + x], len, pm);
            for (int cd = 0; cd < 4; cd++) {
                if (narrow) h_pm32[(size_t)cd * (size_t)nb + (size_t)x] = (uint32_t)pm[cd];
                else h_pm[(size_t)cd * (size_t)nb + (size_t)x] = pm[cd];
            }
            h_len[(size_t)x] = (uint32_t)len;
        }
        // the split of the key list: enough workgroups to fill the device when the pieces alone do not, at least 64 keys each
        const int pblocks = (nb + kOntBlock - 1) / kOntBlock;
        int kpb = forced > 0 ? forced : std::max(64, (c->ont_n + std::max(1, 2048 / pblocks) - 1) / std::max(1, 2048 / pblocks));
        kpb = std::max(kpb, (c->ont_n + 65534) / 65535);               // (gridDim.y)
        const int splits = (c->ont_n + kpb - 1) / kpb;
        if ((rc = ont_dev(c, hipMemcpyAsync(d_pm, h_pm.data(), (narrow ? sizeof(uint32_t) : sizeof(uint64_t)) * 4 * (size_t)nb, hipMemcpyHostToDevice, c->stream), who, "copy")) ||
            (rc = ont_dev(c, hipMemcpyAsync(d_len, h_len.data(), sizeof(uint32_t) * (size_t)nb, hipMemcpyHostToDevice, c->stream), who, "copy")) ||
            (rc = ont_dev(c, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * (size_t)nb, c->stream), who, "hipMemsetAsync")))
            break;
        hipEvent_t ev[2] = {nullptr, nullptr};
        float ms = 0;
        if ((rc = ont_dev(c, hipEventCreate(&ev[0]), who, "hipEventCreate")) == MP_OK && (rc = ont_dev(c, hipEventCreate(&ev[1]), who, "hipEventCreate")) == MP_OK &&
            (rc = ont_dev(c, hipEventRecord(ev[0], c->stream), who, "hipEventRecord")) == MP_OK) {
            if (narrow)
                hipLaunchKernelGGL(ont_assign_kernel<uint32_t>, dim3((unsigned)pblocks, (unsigned)splits), dim3(kOntBlock), 0, c->stream,
                                   (const uint32_t *)d_pm, (const uint32_t *)d_len, nb, (const uint64_t *)c->ont_keys, (int)c->ont_n, kpb,
                                   (const int32_t *)c->ont_q, prune, d_out);
            else
                hipLaunchKernelGGL(ont_assign_kernel<uint64_t>, dim3((unsigned)pblocks, (unsigned)splits), dim3(kOntBlock), 0, c->stream,
                                   (const uint64_t *)d_pm, (const uint32_t *)d_len, nb, (const uint64_t *)c->ont_keys, (int)c->ont_n, kpb,
                                   (const int32_t *)c->ont_q, prune, d_out);
            if ((rc = ont_dev(c, hipGetLastError(), who, "ont_assign_kernel")) == MP_OK &&
                (rc = ont_dev(c, hipEventRecord(ev[1], c->stream), who, "hipEventRecord")) == MP_OK &&
                (rc = ont_dev(c, hipMemcpyAsync(h_out.data(), d_out, sizeof(unsigned long long) * (size_t)nb, hipMemcpyDeviceToHost, c->stream), who, "copy")) == MP_OK &&
                (rc = ont_dev(c, hipStreamSynchronize(c->stream), who, "hipStreamSynchronize")) == MP_OK &&
                (rc = ont_dev(c, hipEventElapsedTime(&ms, ev[0], ev[1]), who, "hipEventElapsedTime")) == MP_OK)
                c->ont_ms += ms;
        }
        for (auto &x : ev) if (x) (void)hipEventDestroy(x);
        if (rc) break;
        for (int x = 0; x < nb; x++) {
            const unsigned long long v = h_out[(size_t)x];
            key[p0 + x] = (int32_t)(0xFFFFFFFFu - (uint32_t)((v >> 8) & 0xFFFFFFFFull));
            m[p0 + x] = (int32_t)(v & 0xFF);
        }
    }
    (void)hipStreamSynchronize(c->stream);
    dev_free(c, &d_pm, cap * 4); dev_free(c, &d_len, cap); dev_free(c, &d_out, cap);
    if (rc == MP_OK) c->ont_counts[1] += n_pieces;
    return rc;
}

int mp_ont_stats(mp_ctx *c, double *ms, int64_t *counts) {
    if (!c) return MP_ERR_ARG;
    if (ms) ms[0] = c->ont_ms;
    if (counts) { counts[0] = c->ont_counts[0]; counts[1] = c->ont_counts[1]; }
    return MP_OK;
}

}  // extern "C"
