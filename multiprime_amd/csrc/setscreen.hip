// setscreen.hip — part of libmprime_hip.so: hand-written HIP (gfx950 / MI355X, wave64) behind include/mprime_setscreen.h, where the rule
// and the three stages are described.  In short:
//
//   scan     kmm_kernel (kmm.hpp) with the sink SsAppend: de-duplicated per-primer site records appended to a list that lives with the
//            context; slots are handed out per wave; nothing is written past the capacity (counted, and the scan runs again at the exact size).
//   bin      counting sort of the reverse sites of one join side by store offset >> shift (ss_bin_count / ss_bin_scan / ss_bin_scatter).
//   join     ss_join_kernel: a thread per forward site, the few bins that cover its size range, products counted per ordered primer pair
//            in an LDS table per workgroup and flushed with one global atomic per (workgroup, pair) into the pair table (open addressing,
//            64-bit keys and counts).  A pair without a slot raises a flag: the host regrows the table and joins again.
//
// No launch depends on a size the device decides: every buffer is allocated from a count the host has read, and every write is guarded by it.
#include "common.hpp"
#include "kmm.hpp"
#include "../../include/mprime_setscreen.h"

#include <tuple>

using namespace mp;

namespace mp {

struct SsSite { long long off; int32_t primer; int32_t rs; };     // store offset of the leftmost base; rs = row (forward) or ~row (reverse)

struct SsTable {                          // the pair table on the device
    unsigned long long *key = nullptr;    // A << 32 | B; kSsEmpty: free
    unsigned long long *cnt = nullptr;
    unsigned long long *flags = nullptr;  // [0] adds that found no slot, [1] slots taken, [2] the emit cursor
    size_t slots = 0;                     // a power of two
};

struct SetScreen {
    int32_t lo = 0, hi = 0, mm = 0, term = 0;
    bool stale = false;                   // the store went away under the screen, or an add failed half way
    SsSite *sites = nullptr;
    size_t cap = 0, headroom = 0;
    long long n = 0;                      // records held
    unsigned long long *d_n = nullptr;
    KmmBlocks blocks;                     // workgroups of the scan, built when the screen is opened
    SsTable table;
    int32_t next_primer = 0;
    std::vector<int64_t> fwd, rev;        // sites per primer id
    long long n_fwd = 0, n_rev = 0;
    std::vector<int64_t> last_out;        // the triples of the last add, and the arguments that made them
    std::vector<uint8_t> last_key;
    int64_t adds = 0;
    explicit SetScreen(mp_ctx *c) : blocks(c) {}
};

}  // namespace mp

namespace {

constexpr unsigned long long kSsEmpty = ~0ull;
constexpr int kSsLds = 1024;              // slots of a workgroup's LDS table
constexpr int kSsLdsProbes = 8;
constexpr int kSsProbes = 64;             // slots tried in the pair table before the add counts as an overflow
constexpr int kScanTile = kBlock * 8;

// ---- the scan's sink ---------------------------------------------------------------------------------------------------------------------
// A thread of kmm_kernel owns its positions and walks the whole pattern table for each; the table lists the reads of a primer contiguously
// (strands interleaved), so per strand a repeat of (position, primer) can only follow the record it repeats.
struct SsAppend {
    struct State { long long p0, p1; int id0, id1; };
    SsSite *sites;
    long long cap;
    unsigned long long *n;                // records asked for (exact, also past cap)
    const int64_t *roff;
    __device__ State begin() const { return {-1, -1, -1, -1}; }
    __device__ void hit(State &st, int row, long long p, int id, int strand) const {
        if (strand) { if (st.p1 == p && st.id1 == id) return; st.p1 = p; st.id1 = id; }
        else { if (st.p0 == p && st.id0 == id) return; st.p0 = p; st.id0 = id; }
        // one atomic per wave: the lanes that are here together take consecutive slots from the first of them
        const unsigned long long act = __ballot(1);
        const int lane = __lane_id();
        unsigned long long base = 0;
        if (lane == __ffsll((long long)act) - 1) base = atomicAdd(n, (unsigned long long)__popcll(act));
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)base), hi = __builtin_amdgcn_readfirstlane((unsigned)(base >> 32));
        const unsigned long long idx = (((unsigned long long)hi << 32) | lo) + (unsigned long long)__popcll(act & ((1ull << lane) - 1ull));
        if ((long long)idx < cap) sites[idx] = SsSite{roff[row] + p, id, strand ? ~row : row};
    }
    __device__ void end(State &, int) const {}
};

// ---- the pair table ------------------------------------------------------------------------------------------------------------------------
__device__ inline unsigned long long ss_hash(unsigned long long x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

__device__ void ss_table_add(const SsTable &T, unsigned long long key, unsigned long long cnt) {
    const unsigned long long mask = T.slots - 1;
    unsigned long long h = ss_hash(key) & mask;
    const int limit = (int)min((unsigned long long)kSsProbes, (unsigned long long)T.slots);
    for (int t = 0; t < limit; t++) {
        const unsigned long long old = atomicCAS(T.key + h, kSsEmpty, key);
        if (old == kSsEmpty) atomicAdd(T.flags + 1, 1ull);
        if (old == kSsEmpty || old == key) { atomicAdd(T.cnt + h, cnt); return; }
        h = (h + 1) & mask;
    }
    atomicAdd(T.flags, 1ull);
}

__device__ void ss_lds_add(unsigned long long *s_key, unsigned long long *s_cnt, const SsTable &T, unsigned long long key, unsigned long long cnt) {
    unsigned h = (unsigned)ss_hash(key) & (kSsLds - 1);
    for (int t = 0; t < kSsLdsProbes; t++) {
        const unsigned long long old = atomicCAS(s_key + h, kSsEmpty, key);
        if (old == kSsEmpty || old == key) { atomicAdd(s_cnt + h, cnt); return; }
        h = (h + 1) & (kSsLds - 1);
    }
    ss_table_add(T, key, cnt);
}

// ---- bin: the reverse sites of [i0, i1) by store offset >> shift ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ss_bin_count_kernel(const SsSite *__restrict__ s, long long i0, long long i1, int shift, long long n_bins,
                                                              unsigned *__restrict__ cnt) {
    const long long i = i0 + (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= i1 || s[i].rs >= 0) return;
    const long long b = s[i].off >> shift;
    if (b < n_bins) atomicAdd(cnt + b, 1u);
}

// exclusive scan by one workgroup: start[b] and cnt[b] (the scatter's cursor) = records in the bins below b, start[n_bins] = all
__global__ __launch_bounds__(kBlock) void ss_bin_scan_kernel(unsigned *__restrict__ cnt, long long n_bins, unsigned *__restrict__ start) {
    __shared__ unsigned s_w[4];
    const int lane = __lane_id(), w = threadIdx.x >> 6;
    unsigned carry = 0;
    for (long long t = 0; t < n_bins; t += kScanTile) {
        const long long j0 = t + threadIdx.x * 8;
        unsigned e[8], v = 0;
        for (int j = 0; j < 8; j++) { e[j] = j0 + j < n_bins ? cnt[j0 + j] : 0u; v += e[j]; }
        unsigned x = v;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        __syncthreads();
        if (lane == 63) s_w[w] = x;
        __syncthreads();
        unsigned before = 0;
        for (int i = 0; i < w; i++) before += s_w[i];
        unsigned run = carry + before + x - v;
        for (int j = 0; j < 8; j++) {
            if (j0 + j < n_bins) { start[j0 + j] = run; cnt[j0 + j] = run; }
            run += e[j];
        }
        carry += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    }
    if (threadIdx.x == 0) start[n_bins] = carry;
}

__global__ __launch_bounds__(kBlock) void ss_bin_scatter_kernel(const SsSite *__restrict__ s, long long i0, long long i1, int shift, long long n_bins,
                                                                unsigned *__restrict__ cur, long long n_slots, long long *__restrict__ r_off,
                                                                int32_t *__restrict__ r_primer) {
    const long long i = i0 + (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= i1 || s[i].rs >= 0) return;
    const long long b = s[i].off >> shift;
    if (b >= n_bins) return;
    const unsigned slot = atomicAdd(cur + b, 1u);
    if ((long long)slot < n_slots) { r_off[slot] = s[i].off; r_primer[slot] = s[i].primer; }
}

// ---- join: the forward sites of [i0, i1) against the binned reverse sites ----------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ss_join_kernel(const SsSite *__restrict__ s, long long i0, long long i1, const int64_t *__restrict__ roff,
                                                         int shift, long long n_bins, const unsigned *__restrict__ start,
                                                         const long long *__restrict__ r_off, const int32_t *__restrict__ r_primer, long long lo,
                                                         long long hi, SsTable T) {
    __shared__ unsigned long long s_key[kSsLds], s_cnt[kSsLds];
    for (int t = threadIdx.x; t < kSsLds; t += kBlock) { s_key[t] = kSsEmpty; s_cnt[t] = 0; }
    __syncthreads();
    const long long i = i0 + (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < i1 && s[i].rs >= 0) {
        const SsSite a = s[i];
        // lo < b - a + 1 < hi  <=>  a + lo <= b <= a + hi - 2, and b on a's row
        const long long from = max(a.off + lo, (long long)roff[a.rs]), to = min(a.off + hi - 2, (long long)roff[a.rs + 1] - 1);
        if (from <= to) {
            unsigned long long cur_key = kSsEmpty, cur_cnt = 0;
            const unsigned long long A = (unsigned long long)(uint32_t)a.primer << 32;
            const long long b1 = min(to >> shift, n_bins - 1);
            for (long long b = from >> shift; b <= b1; b++) {
                const unsigned e1 = start[b + 1];
                for (unsigned j = start[b]; j < e1; j++) {
                    const long long o = r_off[j];
                    if (o < from || o > to) continue;
                    const unsigned long long key = A | (uint32_t)r_primer[j];
                    if (key == cur_key) { cur_cnt++; continue; }
                    if (cur_cnt) ss_lds_add(s_key, s_cnt, T, cur_key, cur_cnt);
                    cur_key = key; cur_cnt = 1;
                }
            }
            if (cur_cnt) ss_lds_add(s_key, s_cnt, T, cur_key, cur_cnt);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kSsLds; t += kBlock)
        if (s_key[t] != kSsEmpty) ss_table_add(T, s_key[t], s_cnt[t]);
}

__global__ __launch_bounds__(kBlock) void ss_emit_kernel(SsTable T, long long cap, long long *__restrict__ out) {
    const size_t h = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (h >= T.slots || T.key[h] == kSsEmpty) return;
    const unsigned long long idx = atomicAdd(T.flags + 2, 1ull);
    if ((long long)idx < cap) {
        out[3 * idx] = (long long)(T.key[h] >> 32); out[3 * idx + 1] = (long long)(T.key[h] & 0xffffffffull); out[3 * idx + 2] = (long long)T.cnt[h];
    }
}

__global__ __launch_bounds__(kBlock) void ss_site_count_kernel(const SsSite *__restrict__ s, long long i0, long long i1, int first, int n_p,
                                                               unsigned long long *__restrict__ cnt) {
    const long long i = i0 + (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= i1) return;
    const long long k = (long long)s[i].primer - first;
    if (k >= 0 && k < n_p) atomicAdd(cnt + (s[i].rs < 0 ? n_p : 0) + k, 1ull);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
long long env_count(const char *name, long long dflt) {
    if (const char *v = getenv(name)) { const long long x = atoll(v); if (x > 0) return x; }
    return dflt;
}

size_t pow2_ceil(unsigned long long x) {
    size_t p = 1;
    while (p < x && p < ((size_t)1 << 40)) p <<= 1;
    return p;
}

void table_free(mp_ctx *c, SsTable &T) {
    dev_free(c, &T.key, T.slots); dev_free(c, &T.cnt, T.slots); dev_free(c, &T.flags, 3);
    T.slots = 0;
}

int table_alloc(mp_ctx *c, SsTable &T, size_t slots) {
    table_free(c, T);
    int rc;
    T.slots = slots;
    if ((rc = dev_alloc(c, &T.key, slots)) || (rc = dev_alloc(c, &T.cnt, slots)) || (rc = dev_alloc(c, &T.flags, 3))) { table_free(c, T); return rc; }
    return MP_OK;
}

int table_clear(mp_ctx *c, SsTable &T) {
    HIPCK(c, hipMemsetAsync(T.key, 0xff, sizeof(unsigned long long) * T.slots, c->stream));
    HIPCK(c, hipMemsetAsync(T.cnt, 0, sizeof(unsigned long long) * T.slots, c->stream));
    HIPCK(c, hipMemsetAsync(T.flags, 0, sizeof(unsigned long long) * 3, c->stream));
    return MP_OK;
}

struct JoinSide { long long f0, f1, r0, r1; };      // forward sites among [f0, f1) against reverse sites among [r0, r1)

// one side: bin, then join into T (T is cleared by the caller)
int join_side(mp_ctx *c, const SsSite *sites, const JoinSide &J, const int64_t *d_roff, long long total, long long lo, long long hi, SsTable &T,
              double *ms) {
    if (J.f1 <= J.f0 || J.r1 <= J.r0) return MP_OK;
    int shift = 0;
    while ((1ll << shift) < MP_SETSCREEN_BIN) shift++;
    while ((total >> shift) + 1 > MP_SETSCREEN_MAX_BINS) shift++;
    const long long n_bins = (total >> shift) + 1, n_r = J.r1 - J.r0;
    if (n_r >= 0xffffffffll) return fail(c, MP_ERR_CAPACITY, "set screen: %lld reverse sites on one join side (fewer than 2^32 supported)", n_r);
    DevBuf<unsigned> cnt(c), start(c);
    DevBuf<long long> r_off(c);
    DevBuf<int32_t> r_primer(c);
    int rc;
    if ((rc = cnt.alloc((size_t)n_bins)) || (rc = start.alloc((size_t)n_bins + 1)) || (rc = r_off.alloc((size_t)n_r)) || (rc = r_primer.alloc((size_t)n_r))) return rc;
    StageClock bin, join;
    bin.begin(c);
    HIPCK(c, cnt.zero());
    hipLaunchKernelGGL(ss_bin_count_kernel, dim3(grid(n_r, kBlock)), dim3(kBlock), 0, c->stream, sites, J.r0, J.r1, shift, n_bins, cnt.p);
    hipLaunchKernelGGL(ss_bin_scan_kernel, dim3(1), dim3(kBlock), 0, c->stream, cnt.p, n_bins, start.p);
    hipLaunchKernelGGL(ss_bin_scatter_kernel, dim3(grid(n_r, kBlock)), dim3(kBlock), 0, c->stream, sites, J.r0, J.r1, shift, n_bins, cnt.p, n_r, r_off.p,
                       r_primer.p);
    HIPCK(c, hipGetLastError());
    bin.end(c);
    join.begin(c);
    hipLaunchKernelGGL(ss_join_kernel, dim3(grid(J.f1 - J.f0, kBlock)), dim3(kBlock), 0, c->stream, sites, J.f0, J.f1, d_roff, shift, n_bins,
                       (const unsigned *)start.p, (const long long *)r_off.p, (const int32_t *)r_primer.p, lo, hi, T);
    HIPCK(c, hipGetLastError());
    join.end(c);
    HIPCK(c, hipStreamSynchronize(c->stream));
    bin.read(ms + 1);
    join.read(ms + 2);
    return MP_OK;
}

// every side into T, regrown and joined again while a pair finds no slot; the triples to `out`
int join_all(mp_ctx *c, const SsSite *sites, const JoinSide *sides, int n_sides, const int64_t *d_roff, long long total, long long lo, long long hi,
             SsTable &T, std::vector<int64_t> &out, double *ms, int64_t *counts) {
    int rc;
    unsigned long long flags[3];
    for (;;) {
        if ((rc = table_clear(c, T))) return rc;
        for (int k = 0; k < n_sides; k++)
            if ((rc = join_side(c, sites, sides[k], d_roff, total, lo, hi, T, ms))) return rc;
        HIPCK(c, hipMemcpyAsync(flags, T.flags, sizeof flags, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        if (!flags[0]) break;
        const size_t want = pow2_ceil(2 * (flags[0] + flags[1]));
        const size_t slots = std::max(2 * T.slots, std::min(16 * T.slots, want));
        if ((rc = table_alloc(c, T, slots))) return rc;
        counts[2]++;
    }
    const size_t n = (size_t)flags[1];
    out.assign(3 * n, 0);
    if (n) {
        DevBuf<long long> d_out(c);
        if ((rc = d_out.alloc(3 * n))) return rc;
        hipLaunchKernelGGL(ss_emit_kernel, dim3(grid((long long)T.slots, kBlock)), dim3(kBlock), 0, c->stream, T, (long long)n, d_out.p);
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipMemcpyAsync(out.data(), d_out.p, sizeof(long long) * 3 * n, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
    }
    counts[5] = (int64_t)n;
    counts[6] = 0;
    for (size_t i = 0; i < n; i++) counts[6] += out[3 * i + 2];
    return MP_OK;
}

int copy_triples(const std::vector<int64_t> &all, int64_t cap, int64_t *out, int64_t *n_out) {
    const int64_t n = (int64_t)(all.size() / 3);
    *n_out = n;
    const int64_t k = std::min<int64_t>(cap, n);
    if (k > 0) memcpy(out, all.data(), sizeof(int64_t) * 3 * (size_t)k);
    return MP_OK;
}

void release_device(mp_ctx *c, SetScreen *S) {
    dev_free(c, &S->sites, S->cap); dev_free(c, &S->d_n, 1);
    S->blocks.release();
    table_free(c, S->table);
    S->cap = 0;
}

// the list with room for `want` records, the first S->n of them kept
int list_reserve(mp_ctx *c, SetScreen *S, size_t want) {
    if (want <= S->cap) return MP_OK;
    DevBuf<SsSite> nl(c);
    int rc;
    if ((rc = nl.alloc(want))) return rc;
    if (S->n) HIPCK(c, hipMemcpyAsync(nl.p, S->sites, sizeof(SsSite) * (size_t)S->n, hipMemcpyDeviceToDevice, c->stream));
    std::swap(nl.p, S->sites);                          // (the old list goes with nl)
    std::swap(nl.n, S->cap);
    return MP_OK;
}

// the scan of one table of new reads into the list from *S->d_n on
int scan_table(mp_ctx *c, SetScreen *S, const KmmTable &T) {
    if (T.n == 0 || S->blocks.size() == 0) return MP_OK;
    DevBuf<uint8_t> d_pats(c);
    int rc;
    if ((rc = d_pats.alloc(T.bytes.size()))) return rc;
    HIPCK(c, d_pats.upload(T.bytes.data(), T.bytes.size()));
    HIPCK(c, kmm_launch<0>(c, kmm_store(c), S->blocks, T, d_pats.p, S->term, SsAppend{S->sites, (long long)S->cap, S->d_n, c->sq_roff}));
    HIPCK(c, hipStreamSynchronize(c->stream));          // (the device table leaves scope)
    return MP_OK;
}

int add_run(mp_ctx *c, SetScreen *S, int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off, const int32_t *read_primer,
            double *ms, int64_t *counts) {
    // one table per kernel form: the reads of a primer have one length, so a primer is whole in one of them
    KmmTable tables[2];
    for (int form = 0; form < 2; form++) {
        std::vector<int32_t> idx;
        for (int32_t i = 0; i < n_pat; i++) if ((pat_off[i + 1] - pat_off[i] > 32) == (form == 1)) idx.push_back(i);
        tables[form] = kmm_table(idx, pat_codes, pat_off, read_primer, S->term);
        tables[form].budget = S->mm;
    }
    const long long n_old = S->n;
    int rc;
    if ((rc = list_reserve(c, S, (size_t)n_old + S->headroom))) return rc;
    unsigned long long n_total = 0;
    for (int pass = 0;; pass++) {
        const unsigned long long h_old = (unsigned long long)n_old;
        HIPCK(c, hipMemcpyAsync(S->d_n, &h_old, sizeof h_old, hipMemcpyHostToDevice, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        StageClock scan;
        scan.begin(c);
        if ((rc = scan_table(c, S, tables[0])) || (rc = scan_table(c, S, tables[1]))) return rc;
        scan.end(c);
        counts[0] += (tables[0].n ? 1 : 0) + (tables[1].n ? 1 : 0);
        HIPCK(c, hipMemcpyAsync(&n_total, S->d_n, sizeof n_total, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        scan.read(ms);
        if (n_total <= S->cap) break;
        if (pass) return fail(c, MP_ERR_DEVICE, "set screen: the scan asked for %llu records after it was given %zu", n_total, S->cap);
        if ((rc = list_reserve(c, S, (size_t)n_total))) return rc;      // the exact size; the records written so far are written again
        counts[1]++;
    }
    S->n = (long long)n_total;
    // sites per new primer
    const int32_t first = read_primer[0], n_p = read_primer[n_pat - 1] - first + 1;
    std::vector<unsigned long long> h_cnt(2 * (size_t)n_p, 0);
    if (S->n > n_old) {
        DevBuf<unsigned long long> d_cnt(c);
        if ((rc = d_cnt.alloc(2 * (size_t)n_p))) return rc;
        HIPCK(c, d_cnt.zero());
        hipLaunchKernelGGL(ss_site_count_kernel, dim3(grid(S->n - n_old, kBlock)), dim3(kBlock), 0, c->stream, (const SsSite *)S->sites, n_old, S->n,
                           (int)first, (int)n_p, d_cnt.p);
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipMemcpyAsync(h_cnt.data(), d_cnt.p, sizeof(unsigned long long) * h_cnt.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
    }
    S->fwd.resize((size_t)first + n_p, 0);
    S->rev.resize((size_t)first + n_p, 0);
    for (int32_t k = 0; k < n_p; k++) {
        S->fwd[(size_t)first + k] = (int64_t)h_cnt[(size_t)k]; S->rev[(size_t)first + k] = (int64_t)h_cnt[(size_t)n_p + k];
        S->n_fwd += (long long)h_cnt[(size_t)k]; S->n_rev += (long long)h_cnt[(size_t)n_p + k];
    }
    S->next_primer = first + n_p;
    // new forward x all reverse, old forward x new reverse
    const JoinSide sides[2] = {{n_old, S->n, 0, S->n}, {0, n_old, n_old, S->n}};
    return join_all(c, S->sites, sides, 2, c->sq_roff, (long long)c->sq_total, S->lo, S->hi, S->table, S->last_out, ms, counts);
}

}  // namespace

namespace mp {

// keep_stale: the store is going away (free_seq) — the screen stays open but refuses every add; otherwise the screen itself goes
void free_setscreen(mp_ctx *c, bool keep_stale) {
    SetScreen *S = c->ss;
    if (!S) return;
    release_device(c, S);
    if (keep_stale) { S->stale = true; S->last_out.clear(); S->last_key.clear(); return; }
    delete S;
    c->ss = nullptr;
}

}  // namespace mp

extern "C" {

int mp_setscreen_begin(mp_ctx *c, int32_t size_lo, int32_t size_hi, int32_t max_mm, int32_t term) {
    if (!c) return MP_ERR_ARG;
    if (max_mm < 0 || term < 0) return fail(c, MP_ERR_ARG, "mp_setscreen_begin: bad arguments");
    if (c->ss) return fail(c, MP_ERR_ARG, "mp_setscreen_begin: a set screen is open already (mp_setscreen_end closes it)");
    if (c->sq_n == 0) return fail(c, MP_ERR_ARG, "mp_setscreen_begin: no sequence store (mp_seq_load comes first)");
    HIPCK(c, hipSetDevice(c->dev));
    SetScreen *S = new SetScreen(c);
    S->lo = size_lo; S->hi = size_hi; S->mm = max_mm; S->term = term;
    S->headroom = (size_t)env_count("MP_SETSCREEN_SITES", 1 << 20);
    int rc;
    if ((rc = dev_alloc(c, &S->d_n, 1)) || (rc = S->blocks.build(c->sq_roff_host.data(), c->sq_n)) ||
        (rc = table_alloc(c, S->table, pow2_ceil((unsigned long long)env_count("MP_SETSCREEN_TABLE", 1 << 16))))) {
        release_device(c, S); delete S; return rc;
    }
    hipError_t e = S->blocks.upload();
    const hipError_t waited = hipStreamSynchronize(c->stream);
    S->blocks.drop_host();
    if (e == hipSuccess) e = waited;
    if (e != hipSuccess) { release_device(c, S); delete S; return fail(c, MP_ERR_DEVICE, "mp_setscreen_begin: %s", hipGetErrorString(e)); }
    for (int i = 0; i < 4; i++) c->ss_ms[i] = 0;
    for (int i = 0; i < 8; i++) c->ss_counts[i] = 0;
    c->ss = S;
    return MP_OK;
}

int mp_setscreen_add(mp_ctx *c, int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off, const int32_t *read_primer, int64_t cap,
                     int64_t *out, int64_t *n_out) {
    if (!c) return MP_ERR_ARG;
    if (n_pat < 0 || !n_out || cap < 0 || (cap && !out) || (n_pat && (!pat_codes || !pat_off || !read_primer)))
        return fail(c, MP_ERR_ARG, "mp_setscreen_add: bad arguments");
    SetScreen *S = c->ss;
    if (!S) return fail(c, MP_ERR_ARG, "mp_setscreen_add: no set screen is open (mp_setscreen_begin comes first)");
    if (S->stale) return fail(c, MP_ERR_ARG, "mp_setscreen_add: the sequence store of this set screen is gone, or an add failed (mp_setscreen_end, then begin again)");
    HIPCK(c, hipSetDevice(c->dev));
    const auto t0 = std::chrono::steady_clock::now();
    *n_out = 0;
    if (n_pat == 0) return MP_OK;
    if (int rc = kmm_check_patterns(c, n_pat, pat_codes, pat_off, [&](int32_t i) {
            if (read_primer[i] < 0 || (i && read_primer[i] < read_primer[i - 1]))
                return fail(c, MP_ERR_ARG, "mp_setscreen_add: read_primer must be non-negative and non-decreasing (read %d)", i);
            if (i && read_primer[i] == read_primer[i - 1] && pat_off[i + 1] - pat_off[i] != pat_off[i] - pat_off[i - 1])
                return fail(c, MP_ERR_ARG, "mp_setscreen_add: the reads of primer %d differ in length (read %d)", read_primer[i], i);
            return (int)MP_OK;
        })) return rc;
    std::vector<uint8_t> key;
    put(key, &n_pat, 1);
    put(key, pat_off, (size_t)n_pat + 1);
    put(key, pat_codes + pat_off[0], (size_t)(pat_off[n_pat] - pat_off[0]));
    put(key, read_primer, (size_t)n_pat);
    double *ms = c->ss_ms;
    int64_t *counts = c->ss_counts;
    for (int i = 0; i < 4; i++) ms[i] = 0;
    counts[0] = counts[1] = counts[2] = 0;
    if (!S->last_key.empty() && key == S->last_key) {           // the last add again: its triples are kept
        int rc = copy_triples(S->last_out, cap, out, n_out);
        ms[3] = ms_since(t0);
        return rc;
    }
    if (read_primer[0] < S->next_primer)
        return fail(c, MP_ERR_ARG, "mp_setscreen_add: primer id %d is not above the ids of earlier adds (next: %d)", read_primer[0], S->next_primer);
    S->last_key.clear();
    S->last_out.clear();
    int rc = add_run(c, S, n_pat, pat_codes, pat_off, read_primer, ms, counts);
    if (rc != MP_OK) { (void)hipStreamSynchronize(c->stream); S->stale = true; return rc; }
    S->adds++;
    counts[3] = S->n_fwd; counts[4] = S->n_rev; counts[7] = S->adds;
    S->last_key = std::move(key);
    rc = copy_triples(S->last_out, cap, out, n_out);
    ms[3] = ms_since(t0);
    return rc;
}

int mp_setscreen_site_counts(mp_ctx *c, int32_t first, int32_t n, int64_t *forward, int64_t *reverse) {
    if (!c) return MP_ERR_ARG;
    if (first < 0 || n < 0 || (n && (!forward || !reverse))) return fail(c, MP_ERR_ARG, "mp_setscreen_site_counts: bad arguments");
    if (!c->ss) return fail(c, MP_ERR_ARG, "mp_setscreen_site_counts: no set screen is open");
    for (int32_t k = 0; k < n; k++) {
        const size_t id = (size_t)first + (size_t)k;
        forward[k] = id < c->ss->fwd.size() ? c->ss->fwd[id] : 0;
        reverse[k] = id < c->ss->rev.size() ? c->ss->rev[id] : 0;
    }
    return MP_OK;
}

int mp_setscreen_stats(mp_ctx *c, double *ms, int64_t *counts) {
    if (!c) return MP_ERR_ARG;
    if (ms) for (int i = 0; i < 4; i++) ms[i] = c->ss_ms[i];
    if (counts) for (int i = 0; i < 8; i++) counts[i] = c->ss_counts[i];
    return MP_OK;
}

int mp_setscreen_end(mp_ctx *c) {
    if (!c) return MP_ERR_ARG;
    HIPCK(c, hipSetDevice(c->dev));
    (void)hipStreamSynchronize(c->stream);
    free_setscreen(c, false);
    return MP_OK;
}

int mp_setscreen_join(mp_ctx *c, int64_t n_sites, const int32_t *sites, int32_t size_lo, int32_t size_hi, int64_t cap, int64_t *out, int64_t *n_out) {
    if (!c) return MP_ERR_ARG;
    if (n_sites < 0 || !n_out || cap < 0 || (cap && !out) || (n_sites && !sites)) return fail(c, MP_ERR_ARG, "mp_setscreen_join: bad arguments");
    HIPCK(c, hipSetDevice(c->dev));
    const auto t0 = std::chrono::steady_clock::now();
    *n_out = 0;
    double *ms = c->ss_ms;
    int64_t *counts = c->ss_counts;
    for (int i = 0; i < 4; i++) ms[i] = 0;
    for (int i = 0; i < 8; i++) counts[i] = 0;
    if (n_sites == 0) return MP_OK;
    // dense rows: the occupied rows in ascending order, each as long as its largest position + 1
    std::vector<int32_t> rows;
    for (int64_t i = 0; i < n_sites; i++) {
        const int32_t *s = sites + 4 * i;
        if ((s[0] != 0 && s[0] != 1) || s[1] < 0 || s[2] < 0 || s[3] < 0)
            return fail(c, MP_ERR_ARG, "mp_setscreen_join: site %lld is not {0|1, row >= 0, pos >= 0, primer >= 0}", (long long)i);
        if (i) {
            const int32_t *p = s - 4;
            if (std::make_tuple(p[0], p[1], p[2], p[3]) >= std::make_tuple(s[0], s[1], s[2], s[3]))
                return fail(c, MP_ERR_ARG, "mp_setscreen_join: sites must ascend strictly in (strand, row, position, primer) (site %lld)", (long long)i);
        }
        rows.push_back(s[1]);
    }
    std::sort(rows.begin(), rows.end());
    rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
    const size_t nr = rows.size();
    std::vector<int64_t> roff(nr + 1, 0);
    std::vector<int32_t> dense((size_t)n_sites);
    for (int64_t i = 0; i < n_sites; i++) {
        const int32_t *s = sites + 4 * i;
        const size_t d = (size_t)(std::lower_bound(rows.begin(), rows.end(), s[1]) - rows.begin());
        dense[(size_t)i] = (int32_t)d;
        roff[d + 1] = std::max<int64_t>(roff[d + 1], (int64_t)s[2] + 1);
    }
    for (size_t d = 0; d < nr; d++) roff[d + 1] += roff[d];
    std::vector<SsSite> h((size_t)n_sites);
    for (int64_t i = 0; i < n_sites; i++) {
        const int32_t *s = sites + 4 * i;
        const int32_t d = dense[(size_t)i];
        h[(size_t)i] = SsSite{roff[(size_t)d] + s[2], s[3], s[0] ? ~d : d};
        counts[3 + s[0]]++;
    }
    DevBuf<SsSite> d_sites(c);
    DevBuf<int64_t> d_roff(c);
    SsTable T;
    int rc;
    if ((rc = d_sites.alloc((size_t)n_sites)) || (rc = d_roff.alloc(nr + 1)) ||
        (rc = table_alloc(c, T, pow2_ceil((unsigned long long)env_count("MP_SETSCREEN_TABLE", 1 << 16))))) return rc;
    hipError_t e = hipMemcpyAsync(d_sites.p, h.data(), sizeof(SsSite) * h.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_roff.p, roff.data(), sizeof(int64_t) * roff.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    std::vector<int64_t> all;
    if (e != hipSuccess) rc = fail(c, MP_ERR_DEVICE, "mp_setscreen_join: %s", hipGetErrorString(e));
    else {
        const JoinSide side{0, n_sites, 0, n_sites};
        rc = join_all(c, d_sites.p, &side, 1, d_roff.p, roff[nr], size_lo, size_hi, T, all, ms, counts);
    }
    (void)hipStreamSynchronize(c->stream);
    table_free(c, T);
    if (rc != MP_OK) return rc;
    rc = copy_triples(all, cap, out, n_out);
    ms[3] = ms_since(t0);
    return rc;
}

}  // extern "C"
