// offtarget.hip — part of libmprime_hip.so: hand-written HIP (gfx950 / MI355X, wave64) behind include/mprime_offtarget.h.
// The off-target screen of scripts/primer_specificity.py without the hits ever leaving the device:
//
//   scan     kmm_kernel (kmm.hpp: mp_kmm_scan's rule and pattern table) over the resident store, one launch per mismatch budget.  Its
//            sink folds every hit into a SITE MAP — one uint32 per (strand, base of the store) holding 1 + the largest read index that
//            hit there (atomicMax) — and keeps, per sequence, the smallest read index with a forward hit (a wave minimum, one atomicMin
//            per wave).  The reduction IS the scan: there is no hit list to size, to overflow or to sort.
//   reduce   stream compaction of the map (count per chunk, exclusive scan, stable write): the sites of both strands, ascending in
//            (strand, sequence, position) because the map is laid out that way, each with its read mapped to its primer id; then the
//            first site of every (strand, sequence) by binary search.
//   join     validate.amplicons() per sequence: one thread per forward site counts its stops (binary searches in the sequence's reverse
//            sites), marks the whole-sequence reject and the first start without a stop (atomicMin per sequence); an exclusive scan of
//            the counts; the sequences' order (smallest read with a forward hit, sequence) on the host over the per-sequence totals —
//            O(sequences), no hit or site crosses the bus —; then one thread per start writes its products.
//
// mp_amplicon_join runs the join on explicit sites (position key row << 32 | position instead of the store's offsets).
#include "common.hpp"
#include "kmm.hpp"
#include "../../include/mprime_offtarget.h"

using namespace mp;

namespace {

constexpr int kChunk = kBlock * 16;              // map entries per workgroup of the compaction
constexpr int kScanTile = kBlock * 8;            // elements per workgroup of the exclusive scan
constexpr int kOtCounts = 7;                     // mp_offtarget_stats counts

// ---- the scan's sink ---------------------------------------------------------------------------------------------------------------
struct OtSites {
    struct State { int mn; unsigned hits; };
    uint32_t *map;                    // [2][n_bases]: forward half, reverse half
    const int64_t *roff;              // the store's byte offsets
    long long n_bases;
    int32_t *row_min;                 // [n_rows] smallest read with a forward hit (0x7fffffff: none)
    unsigned long long *n_hits;
    __device__ State begin() const { return {0x7fffffff, 0u}; }
    __device__ void hit(State &st, int row, long long p, int id, int strand) const {
        atomicMax(map + (strand ? n_bases : 0) + roff[row] + p, (uint32_t)id + 1u);
        if (!strand) st.mn = min(st.mn, id);
        st.hits++;
    }
    __device__ void end(State &st, int row) const {     // the whole wave arrives here (one row per workgroup)
        int mn = st.mn;
        unsigned h = st.hits;
        for (int o = 32; o > 0; o >>= 1) { mn = min(mn, __shfl_xor(mn, o)); h += __shfl_xor(h, o); }
        if (__lane_id() == 0) {
            if (mn != 0x7fffffff) atomicMin(row_min + row, mn);
            if (h) atomicAdd(n_hits, (unsigned long long)h);
        }
    }
};

// ---- block-wide helpers (kBlock = 256 threads = 4 waves) ------------------------------------------------------------------------------
__device__ long long block_sum(long long v, long long *s_w) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if (__lane_id() == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// exclusive prefix of v over the block in thread order; *total = the block's sum
__device__ long long block_exclusive(long long v, long long *s_w, long long *total) {
    const int lane = __lane_id(), w = threadIdx.x >> 6;
    long long x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const long long y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    __syncthreads();
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    long long before = 0;
    for (int i = 0; i < w; i++) before += s_w[i];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return before + x - v;
}

// ---- exclusive scan of int64 (out[0..n]: out[n] = the total) ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void scan_tiles_kernel(const long long *__restrict__ in, long long n, long long *__restrict__ part) {
    __shared__ long long s_w[4];
    const long long i0 = (long long)blockIdx.x * kScanTile + threadIdx.x * 8;
    long long v = 0;
    for (int j = 0; j < 8; j++) if (i0 + j < n) v += in[i0 + j];
    v = block_sum(v, s_w);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// one tile of kScanTile elements from `start`, with `carry` in front; returns the tile's sum (every thread)
__device__ long long scan_tile(const long long *in, long long *out, long long n, long long start, long long carry, long long *s_w) {
    const long long i0 = start + threadIdx.x * 8;
    long long e[8], v = 0;
    for (int j = 0; j < 8; j++) { e[j] = i0 + j < n ? in[i0 + j] : 0; v += e[j]; }
    long long total;
    long long run = carry + block_exclusive(v, s_w, &total);
    for (int j = 0; j < 8; j++) {
        if (i0 + j < n) out[i0 + j] = run;
        run += e[j];
    }
    return total;
}

// the tile sums, scanned in place by one workgroup; the grand total to *total_out
__global__ __launch_bounds__(kBlock) void scan_parts_kernel(long long *part, long long n_part, long long *__restrict__ total_out) {
    __shared__ long long s_w[4];
    long long carry = 0;
    for (long long t = 0; t < n_part; t += kScanTile) carry += scan_tile(part, part, n_part, t, carry, s_w);
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(kBlock) void scan_apply_kernel(const long long *__restrict__ in, long long n, const long long *__restrict__ part,
                                                            long long *__restrict__ out) {
    __shared__ long long s_w[4];
    (void)scan_tile(in, out, n, (long long)blockIdx.x * kScanTile, part[blockIdx.x], s_w);
}

// ---- reduce: compaction of the site map --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void map_count_kernel(const uint32_t *__restrict__ map, long long n2, long long *__restrict__ cnt) {
    __shared__ long long s_w[4];
    const long long c0 = (long long)blockIdx.x * kChunk;
    long long v = 0;
    for (int r = 0; r < kChunk / kBlock; r++) {
        const long long i = c0 + r * kBlock + threadIdx.x;
        v += i < n2 && map[i] != 0;
    }
    v = block_sum(v, s_w);
    if (threadIdx.x == 0) cnt[blockIdx.x] = v;
}

// the sites of one chunk in map order from base[chunk]: key = map index, primer = read_primer[read]
__global__ __launch_bounds__(kBlock) void map_write_kernel(const uint32_t *__restrict__ map, long long n2, const long long *__restrict__ base,
                                                           const int32_t *__restrict__ read_primer, long long *__restrict__ key,
                                                           int32_t *__restrict__ primer) {
    __shared__ long long s_w[4];
    const long long c0 = (long long)blockIdx.x * kChunk;
    long long run = base[blockIdx.x];
    for (int r = 0; r < kChunk / kBlock; r++) {
        const long long i = c0 + r * kBlock + threadIdx.x;
        const uint32_t m = i < n2 ? map[i] : 0u;
        long long total;
        const long long at = run + block_exclusive(m != 0, s_w, &total);
        if (m) { key[at] = i; primer[at] = read_primer[m - 1]; }
        run += total;
    }
}

__device__ long long lower_bound(const long long *a, long long lo, long long hi, long long x) {     // first index in [lo, hi) with a[i] >= x
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// first site of every (strand, row): f_lo[r] / r_lo[r] for r = 0 .. n_rows (the last entry ends the strand)
__global__ __launch_bounds__(kBlock) void site_rows_kernel(const long long *__restrict__ key, long long n_sites, const int64_t *__restrict__ roff,
                                                           int n_rows, long long n_bases, long long *__restrict__ f_lo, long long *__restrict__ r_lo) {
    const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (r > n_rows) return;
    f_lo[r] = lower_bound(key, 0, n_sites, roff[r]);
    r_lo[r] = lower_bound(key, 0, n_sites, n_bases + roff[r]);
}

// ---- join -------------------------------------------------------------------------------------------------------------------------------
struct JoinArgs {
    const long long *key;             // site keys: forward sites [0, n_fwd) hold the position key, reverse sites hold n_bases + it
    const int32_t *primer;
    const int64_t *roff;              // position key of a row's first base
    int n_rows;
    long long n_bases, n_fwd;
    const long long *f_lo, *r_lo;
    long long lo, hi;                 // the size range
};

__device__ int row_of(const JoinArgs &A, long long k) {      // the row whose range [roff[r], roff[r + 1]) holds k
    int lo = 0, hi = A.n_rows;                                // last r with roff[r] <= k
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (A.roff[mid] <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// per forward site: its row, its number of products before the per-row cuts, and the cuts (whole-row reject, first dead start)
__global__ __launch_bounds__(kBlock) void join_count_kernel(JoinArgs A, int32_t *__restrict__ site_row, long long *__restrict__ cnt,
                                                            int32_t *__restrict__ dead) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.n_fwd) return;
    const long long a = A.key[i];
    const int row = row_of(A, a);
    site_row[i] = row;
    cnt[i] = 0;
    const long long rlo = A.r_lo[row], rhi = A.r_lo[row + 1], flo = A.f_lo[row], fhi = A.f_lo[row + 1];
    if (rlo == rhi) return;                                                   // no reverse site: not a gene of `both`
    const long long t_first = A.key[rlo] - A.n_bases, t_last = A.key[rhi - 1] - A.n_bases;
    if (t_first - A.key[fhi - 1] > A.hi || t_last - A.key[flo] < A.lo) return;  // the whole row gives nothing
    const long long first = lower_bound(A.key, rlo, rhi, A.n_bases + a + A.lo);
    const long long last = a + A.hi > t_last ? rhi - 1 : lower_bound(A.key, rlo, rhi, A.n_bases + a + A.hi) - 1;
    if (first > last) { atomicMin(dead + row, (int32_t)(i - flo)); return; }  // this start and every later one of the row: nothing
    // stop - start + 1 < hi  <=>  stop <= start + hi - 2; from `first` on stop >= start + lo, so the lower bound holds already
    const long long end = lower_bound(A.key, first, rhi, A.n_bases + a + A.hi - 1);
    cnt[i] = end - first;
}

__global__ __launch_bounds__(kBlock) void join_cut_kernel(JoinArgs A, const int32_t *__restrict__ site_row, const int32_t *__restrict__ dead,
                                                          long long *__restrict__ cnt) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.n_fwd) return;
    const int row = site_row[i];
    if (i - A.f_lo[row] >= dead[row]) cnt[i] = 0;
}

// products per row (off = the exclusive scan of the counts, n_fwd + 1 entries); rows with forward / reverse / both kinds of sites
__global__ __launch_bounds__(kBlock) void join_rows_kernel(JoinArgs A, const long long *__restrict__ off, long long *__restrict__ total,
                                                           unsigned long long *__restrict__ genes) {
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= A.n_rows) return;
    total[r] = off[A.f_lo[r + 1]] - off[A.f_lo[r]];
    const bool f = A.f_lo[r + 1] > A.f_lo[r], b = A.r_lo[r + 1] > A.r_lo[r];
    if (f) atomicAdd(genes, 1ull);
    if (b) atomicAdd(genes + 1, 1ull);
    if (f && b) atomicAdd(genes + 2, 1ull);
}

__global__ __launch_bounds__(kBlock) void join_emit_kernel(JoinArgs A, const int32_t *__restrict__ site_row, const long long *__restrict__ off,
                                                           const long long *__restrict__ row_base, int32_t *__restrict__ out) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.n_fwd) return;
    const long long n = off[i + 1] - off[i];
    if (n == 0) return;
    const int row = site_row[i];
    const long long a = A.key[i], r0 = A.roff[row];
    const long long first = lower_bound(A.key, A.r_lo[row], A.r_lo[row + 1], A.n_bases + a + A.lo);
    int32_t *o = out + 6 * (row_base[row] + off[i] - off[A.f_lo[row]]);
    for (long long j = 0; j < n; j++, o += 6) {
        const long long b = A.key[first + j] - A.n_bases;
        o[0] = row; o[1] = (int32_t)(a - r0); o[2] = (int32_t)(b - r0); o[3] = A.primer[i]; o[4] = A.primer[first + j]; o[5] = (int32_t)(b - a + 1);
    }
}

// exclusive scan of n int64 into out[0..n] (device arrays; `out` may not alias `in`)
int scan_i64(mp_ctx *c, const long long *in, long long n, long long *out) {
    const long long n_part = (n + kScanTile - 1) / kScanTile;
    DevBuf<long long> part(c);
    int rc;
    if ((rc = part.alloc((size_t)n_part + 1))) return rc;
    if (n_part) hipLaunchKernelGGL(scan_tiles_kernel, dim3(grid(n, kScanTile)), dim3(kBlock), 0, c->stream, in, n, part.p);
    hipLaunchKernelGGL(scan_parts_kernel, dim3(1), dim3(kBlock), 0, c->stream, part.p, n_part, out + n);
    if (n_part) hipLaunchKernelGGL(scan_apply_kernel, dim3(grid(n, kScanTile)), dim3(kBlock), 0, c->stream, in, n, (const long long *)part.p, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, MP_ERR_DEVICE, "scan: %s", hipGetErrorString(e));
    return MP_OK;
}

// the six-column products on the device go: another call's, or this call's once they were copied out
void drop_products(mp_ctx *c) {
    dev_free(c, &c->ot_out, (size_t)c->ot_n * 6);
    c->ot_n = 0;
}

// Everything after the sites: sites [0, n_fwd) forward, [n_fwd, n_sites) reverse (key n_bases + position key), rows keyed by row_key
// (int32 per row: the sequence order is ascending (row_key, row)).  Products into c->ot_out (c->ot_n of them).
int join_device(mp_ctx *c, const long long *d_key, const int32_t *d_primer, long long n_sites, const int64_t *d_roff, int n_rows,
                long long n_bases, const int32_t *d_row_key, int32_t size_lo, int32_t size_hi) {
    DevBuf<long long> f_lo(c), r_lo(c), rtot(c), rbase(c), cnt(c), off(c);
    DevBuf<int32_t> dead(c), site_row(c);
    DevBuf<unsigned long long> genes(c);
    const size_t nr1 = (size_t)n_rows + 1;
    int rc;
    if ((rc = f_lo.alloc(nr1)) || (rc = r_lo.alloc(nr1)) || (rc = rtot.alloc(nr1)) || (rc = rbase.alloc(nr1)) || (rc = dead.alloc(nr1)) ||
        (rc = genes.alloc(3))) return rc;
    hipLaunchKernelGGL(site_rows_kernel, dim3(grid(n_rows + 1, kBlock)), dim3(kBlock), 0, c->stream, d_key, n_sites, d_roff, n_rows, n_bases, f_lo.p, r_lo.p);
    HIPCK_WAIT(c, hipGetLastError());
    long long n_fwd = 0;
    HIPCK_WAIT(c, hipMemcpyAsync(&n_fwd, f_lo.p + n_rows, sizeof n_fwd, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->ot_counts[1] = n_fwd;
    c->ot_counts[2] = n_sites - n_fwd;
    JoinArgs A{d_key, d_primer, d_roff, n_rows, n_bases, n_fwd, f_lo.p, r_lo.p, size_lo, size_hi};
    const size_t nf = (size_t)std::max<long long>(n_fwd, 1);
    if ((rc = site_row.alloc(nf)) || (rc = cnt.alloc(nf)) || (rc = off.alloc(nf + 1))) return rc;
    FillSeg segs[2] = {{dead.p, nr1 * 4, 0x7fffffffu}, {genes.p, 3 * sizeof(unsigned long long), 0u}};
    if ((rc = fill_segments(c, segs, 2))) return rc;
    if (n_fwd) {
        hipLaunchKernelGGL(join_count_kernel, dim3(grid(n_fwd, kBlock)), dim3(kBlock), 0, c->stream, A, site_row.p, cnt.p, dead.p);
        hipLaunchKernelGGL(join_cut_kernel, dim3(grid(n_fwd, kBlock)), dim3(kBlock), 0, c->stream, A, (const int32_t *)site_row.p, (const int32_t *)dead.p, cnt.p);
        HIPCK_WAIT(c, hipGetLastError());
    }
    if ((rc = scan_i64(c, cnt.p, n_fwd, off.p))) return rc;
    hipLaunchKernelGGL(join_rows_kernel, dim3(grid(n_rows, kBlock)), dim3(kBlock), 0, c->stream, A, (const long long *)off.p, rtot.p, genes.p);
    HIPCK_WAIT(c, hipGetLastError());
    // the sequence order: per-row totals and keys to the host (O(rows)), sorted there, the bases back
    std::vector<long long> h_tot((size_t)n_rows), h_base((size_t)n_rows, 0);
    std::vector<int32_t> h_key((size_t)n_rows);
    unsigned long long h_genes[3] = {0, 0, 0};
    if (n_rows) {
        HIPCK_WAIT(c, hipMemcpyAsync(h_tot.data(), rtot.p, sizeof(long long) * n_rows, hipMemcpyDeviceToHost, c->stream));
        HIPCK_WAIT(c, hipMemcpyAsync(h_key.data(), d_row_key, sizeof(int32_t) * n_rows, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCK_WAIT(c, hipMemcpyAsync(h_genes, genes.p, sizeof h_genes, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 3; i++) c->ot_counts[4 + i] = (int64_t)h_genes[i];
    std::vector<std::pair<int32_t, int32_t>> order;
    for (int r = 0; r < n_rows; r++) if (h_tot[(size_t)r]) order.push_back({h_key[(size_t)r], r});
    std::sort(order.begin(), order.end());
    long long total = 0;
    for (auto &kr : order) { h_base[(size_t)kr.second] = total; total += h_tot[(size_t)kr.second]; }
    drop_products(c);
    if ((rc = dev_alloc(c, &c->ot_out, (size_t)std::max<long long>(total, 1) * 6))) return rc;
    c->ot_n = total;
    if (total) {
        HIPCK_WAIT(c, rbase.upload(h_base.data(), (size_t)n_rows));
        hipLaunchKernelGGL(join_emit_kernel, dim3(grid(n_fwd, kBlock)), dim3(kBlock), 0, c->stream, A, (const int32_t *)site_row.p,
                           (const long long *)off.p, (const long long *)rbase.p, c->ot_out);
        HIPCK_WAIT(c, hipGetLastError());
        HIPCK(c, hipStreamSynchronize(c->stream));          // (h_base leaves scope)
    }
    c->ot_counts[3] = total;
    return MP_OK;
}

// the first min(cap, ot_n) kept products to the caller
int copy_out(mp_ctx *c, int64_t cap, int32_t *out, int64_t *n_out) {
    *n_out = c->ot_n;
    const long long n = std::min<long long>(cap, c->ot_n);
    if (n > 0) {
        HIPCK(c, hipMemcpyAsync(out, c->ot_out, sizeof(int32_t) * 6 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
    }
    return MP_OK;
}

// ---- the screen: a scan into a site map, then the map's sites in order ---------------------------------------------------------------
// What both screens do between their arguments and their joins.  The map has `segments` segments of one entry per base of the store;
// which of them a hit lands in is the sink's business.  The block list and the pattern tables live on the host as long as the object:
// their copies are covered by the wait in reduce(), and by the destructor's when a call fails before it.
struct Screen {
    mp_ctx *c;
    const long long n_bases, n_map, n_chunks;
    KmmBlocks blocks;
    std::vector<KmmTable> tables;
    DevBuf<uint32_t> map;
    DevBuf<uint8_t> pats;
    DevBuf<unsigned long long> d_hits;
    DevBuf<long long> ccnt, cbase, key;      // key / primer: the n_sites sites of the map, ascending in map order
    DevBuf<int32_t> primer;
    long long n_sites = 0;
    unsigned long long hits = 0;             // hits of the scan, before the map folded them
    bool in_flight = false;

    Screen(mp_ctx *ctx, int segments)
        : c(ctx), n_bases((long long)ctx->sq_total), n_map(segments * n_bases), n_chunks((n_map + kChunk - 1) / kChunk), blocks(ctx), map(ctx),
          pats(ctx), d_hits(ctx), ccnt(ctx), cbase(ctx), key(ctx), primer(ctx) {}
    ~Screen() { if (in_flight) (void)hipStreamSynchronize(c->stream); }

    // one pattern table per budget (kmm_tables), the workgroups of the store, every buffer whose size the host knows
    int open(int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off, const int32_t *budget, int32_t max_gap, int32_t term) {
        tables = kmm_tables(n_pat, pat_codes, pat_off, budget, max_gap, term);
        int rc;
        if ((rc = blocks.build(c->sq_roff_host.data(), c->sq_n)) || (rc = map.alloc((size_t)n_map)) || (rc = pats.alloc(kmm_table_bytes(tables))) ||
            (rc = d_hits.alloc(1)) || (rc = ccnt.alloc((size_t)n_chunks)) || (rc = cbase.alloc((size_t)n_chunks + 1))) return rc;
        return MP_OK;
    }
    int clear() {
        in_flight = true;
        HIPCK(c, map.zero());
        HIPCK(c, d_hits.zero());
        HIPCK(c, blocks.upload());
        return MP_OK;
    }
    // one launch per table
    template <int FORMS, class Sink> int scan(int32_t term, const Sink &sink) {
        for (auto &T : tables) {
            if (blocks.size() == 0) break;
            // (from the second table on the copy overwrites pats: it waits for the launch before it on the stream)
            HIPCK(c, pats.upload(T.bytes.data(), T.bytes.size()));
            HIPCK(c, kmm_launch<FORMS>(c, kmm_store(c), blocks, T, pats.p, term, sink));
        }
        return MP_OK;
    }
    // the map's sites in order: key = map index, primer = d_read_id[read]
    int reduce(const int32_t *d_read_id) {
        hipLaunchKernelGGL(map_count_kernel, dim3(grid(n_map, kChunk)), dim3(kBlock), 0, c->stream, (const uint32_t *)map.p, n_map, ccnt.p);
        HIPCK(c, hipGetLastError());
        int rc;
        if ((rc = scan_i64(c, ccnt.p, n_chunks, cbase.p))) return rc;
        HIPCK(c, hipMemcpyAsync(&n_sites, cbase.p + n_chunks, sizeof n_sites, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipMemcpyAsync(&hits, d_hits.p, sizeof hits, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));          // (the block list and the pattern tables may go now)
        in_flight = false;
        const size_t ns = (size_t)std::max<long long>(n_sites, 1);
        if ((rc = key.alloc(ns)) || (rc = primer.alloc(ns))) return rc;
        hipLaunchKernelGGL(map_write_kernel, dim3(grid(n_map, kChunk)), dim3(kBlock), 0, c->stream, (const uint32_t *)map.p, n_map,
                           (const long long *)cbase.p, d_read_id, key.p, primer.p);
        HIPCK(c, hipGetLastError());
        return MP_OK;
    }
};

// The screen behind both entry points.  max_gap < 0: mp_offtarget_resident — max_mm[i] is read i's mismatch budget (kmm_kernel);
// max_gap >= 0: mp_offtarget_gap_resident — max_mm[i] is read i's penalty ceiling, and a table whose ceiling admits a gap goes through
// kmm_gap_kernel (the others through kmm_kernel with ceiling / 6 mismatches: the same sites).
int offtarget_run(mp_ctx *c, const char *who, int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off, const int32_t *read_primer,
                  const int32_t *max_mm, int32_t max_gap, int32_t term, int32_t size_lo, int32_t size_hi, int64_t cap, int32_t *out, int64_t *n_out) {
    if (!c) return MP_ERR_ARG;
    if (n_pat < 0 || !n_out || cap < 0 || (cap && !out) || (n_pat && (!pat_codes || !pat_off || !read_primer || !max_mm)) || term < 0)
        return fail(c, MP_ERR_ARG, "%s: bad arguments", who);
    if (max_gap > MP_KMM_MAX_GAP) return fail(c, MP_ERR_ARG, "%s: max_gap %d (0..%d)", who, max_gap, MP_KMM_MAX_GAP);
    HIPCK(c, hipSetDevice(c->dev));
    const auto t0 = std::chrono::steady_clock::now();
    *n_out = 0;
    for (int i = 0; i < 4; i++) c->ot_ms[i] = 0;
    int rc;
    if ((rc = kmm_check_patterns(c, n_pat, pat_codes, pat_off, [&](int32_t i) {
            return max_mm[i] < 0 ? fail(c, MP_ERR_ARG, "pattern %d has a negative %s", i, max_gap < 0 ? "mismatch budget" : "penalty ceiling") : MP_OK;
        }))) return rc;
    if (c->sq_n == 0 || n_pat == 0) {
        for (int i = 0; i < kOtCounts; i++) c->ot_counts[i] = 0;
        drop_products(c);
        c->ot_key.clear();
        return MP_OK;
    }
    // a repeat of the last call (a larger cap after *n_out > cap): its products are still on the device
    std::vector<uint8_t> key;
    const int32_t head[5] = {n_pat, term, size_lo, size_hi, max_gap};
    put(key, head, 5);
    put(key, pat_off, (size_t)n_pat + 1);
    put(key, pat_codes + pat_off[0], (size_t)(pat_off[n_pat] - pat_off[0]));
    put(key, read_primer, (size_t)n_pat);
    put(key, max_mm, (size_t)n_pat);
    if (!c->ot_key.empty() && key == c->ot_key) {
        rc = copy_out(c, cap, out, n_out);
        c->ot_ms[3] = ms_since(t0);
        return rc;
    }
    c->ot_key.clear();
    for (int i = 0; i < kOtCounts; i++) c->ot_counts[i] = 0;
    const int n_rows = c->sq_n;
    Screen X(c, 2);
    DevBuf<int32_t> row_min(c), d_rp(c);
    if ((rc = X.open(n_pat, pat_codes, pat_off, max_mm, max_gap, term)) || (rc = row_min.alloc((size_t)n_rows)) || (rc = d_rp.alloc((size_t)n_pat))) return rc;
    StageClock scan, reduce, join;           // the stage times are device times: one stage ends where the next begins
    scan.begin(c);
    if ((rc = X.clear())) return rc;
    HIPCK(c, d_rp.upload(read_primer, (size_t)n_pat));
    FillSeg seg{row_min.p, sizeof(int32_t) * (size_t)n_rows, 0x7fffffffu};
    if ((rc = fill_segments(c, &seg, 1))) return rc;
    if ((rc = X.scan<kKmmGaps>(term, OtSites{X.map.p, c->sq_roff, X.n_bases, row_min.p, X.d_hits.p}))) return rc;
    scan.end(c);
    reduce.begin(c);
    if ((rc = X.reduce(d_rp.p))) return rc;
    X.map.release();            // the largest block of the call: the join takes it back from the pool (a released block is ordered on the stream)
    reduce.end(c);
    join.begin(c);
    if ((rc = join_device(c, X.key.p, X.primer.p, X.n_sites, c->sq_roff, n_rows, X.n_bases, row_min.p, size_lo, size_hi))) return rc;
    join.end(c);
    join.read(c->ot_ms + 2);
    scan.read(c->ot_ms);
    reduce.read(c->ot_ms + 1);
    c->ot_counts[0] = (int64_t)X.hits;
    c->ot_key = std::move(key);
    rc = copy_out(c, cap, out, n_out);
    c->ot_ms[3] = ms_since(t0);
    return rc;
}

// ---- the class joins of the panel update (include/mprime_panel.h) ----------------------------------------------------------------------
// Sites carry a class (0 core, 1 new); the site map has four segments of n_bases entries, segment = 2 * class + strand, so the compaction
// leaves the sites ascending in (class, strand, sequence, position).  A join takes the forward segment of one class and the reverse
// segment of another: the two slices are copied into one key array in join_device's layout and joined by the kernels above.
constexpr int kJoinClasses = 3;
constexpr int kJoinFwd[kJoinClasses] = {0, 2, 2};          // segment of the forward sites: core, new, new
constexpr int kJoinRev[kJoinClasses] = {3, 1, 3};          // segment of the reverse sites: new, core, new

struct OtClassSites {
    struct State { unsigned hits; };
    uint32_t *map;                    // [4][n_bases]: segment 2 * class + strand
    const int64_t *roff;
    long long n_bases;
    const int32_t *read_class;        // [n_reads] 0 core, 1 new
    unsigned long long *n_hits;
    __device__ State begin() const { return {0u}; }
    __device__ void hit(State &st, int row, long long p, int id, int strand) const {
        atomicMax(map + (long long)(2 * read_class[id] + strand) * n_bases + roff[row] + p, (uint32_t)id + 1u);
        st.hits++;
    }
    __device__ void end(State &st, int) const {
        unsigned h = st.hits;
        for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o);
        if (__lane_id() == 0 && h) atomicAdd(n_hits, (unsigned long long)h);
    }
};

// first site of every segment: bound[s] for s = 0 .. 4
__global__ void segment_bounds_kernel(const long long *__restrict__ key, long long n_sites, long long n_bases, long long *__restrict__ bound) {
    if (threadIdx.x <= 4) bound[threadIdx.x] = lower_bound(key, 0, n_sites, (long long)threadIdx.x * n_bases);
}

// the sites [f_lo, f_lo + n_f) and [r_lo, r_lo + n_r) of the compacted map as one join input: forward keys first, reverse keys at n_bases +
__global__ __launch_bounds__(kBlock) void join_pick_kernel(const long long *__restrict__ key, const int32_t *__restrict__ primer, long long f_lo,
                                                           long long n_f, long long f_sub, long long r_lo, long long n_r, long long r_sub,
                                                           long long n_bases, long long *__restrict__ out_key, int32_t *__restrict__ out_primer) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_f + n_r) return;
    if (i < n_f) { out_key[i] = key[f_lo + i] - f_sub; out_primer[i] = primer[f_lo + i]; }
    else { out_key[i] = key[r_lo + i - n_f] - r_sub + n_bases; out_primer[i] = primer[r_lo + i - n_f]; }
}

// one join through join_device; its products, widened by the class column, are appended to out7 and its counts added to acc[1..6]
int join_one_class(mp_ctx *c, const long long *d_key, const int32_t *d_primer, long long n_sites, const int64_t *d_roff, int n_rows,
                   long long n_bases, const int32_t *d_row_key, int32_t size_lo, int32_t size_hi, int cls, std::vector<int32_t> &out7, int64_t *acc) {
    int rc = join_device(c, d_key, d_primer, n_sites, d_roff, n_rows, n_bases, d_row_key, size_lo, size_hi);
    if (rc != MP_OK) return rc;
    const size_t n = (size_t)c->ot_n;
    std::vector<int32_t> six(n * 6);
    if (n) {
        HIPCK(c, hipMemcpyAsync(six.data(), c->ot_out, sizeof(int32_t) * 6 * n, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
    }
    out7.reserve(out7.size() + n * 7);
    for (size_t i = 0; i < n; i++) {
        out7.insert(out7.end(), six.begin() + 6 * i, six.begin() + 6 * i + 6);
        out7.push_back(cls);
    }
    for (int i = 1; i < kOtCounts; i++) acc[i] += c->ot_counts[i];
    drop_products(c);                                       // the six-column products belong to no store
    return MP_OK;
}

int copy_out7(const std::vector<int32_t> &all, int64_t cap, int32_t *out, int64_t *n_out) {
    const int64_t n = (int64_t)(all.size() / 7);
    *n_out = n;
    const int64_t k = std::min<int64_t>(cap, n);
    if (k > 0) memcpy(out, all.data(), sizeof(int32_t) * 7 * (size_t)k);
    return MP_OK;
}

// ---- explicit sites (mp_amplicon_join, mp_amplicon_join_classes) ---------------------------------------------------------------------
// Sites of w int32 each: w - 3 leading columns of 0 | 1 (strand; class and strand), then row, position and an id, strictly ascending in
// all but the id.  Their rows as a join sees them: position key row << 32 | position, sequences in ascending row order.
struct SiteRows {
    int n_rows = 0;
    long long n_bases = 0;
    std::vector<int32_t> row_key;            // (the host tables live with the object: upload() is covered by the caller's next wait)
    std::vector<int64_t> roff;
    DevBuf<int32_t> d_rkey;
    DevBuf<int64_t> d_roff;
    explicit SiteRows(mp_ctx *c) : d_rkey(c), d_roff(c) {}
    // `shape` and `order` describe a site and its ordering columns in the messages
    int open(const char *who, int64_t n_sites, const int32_t *sites, int w, const char *shape, const char *order) {
        mp_ctx *c = d_rkey.c;
        int32_t max_row = 0;
        for (int64_t i = 0; i < n_sites; i++) {
            const int32_t *s = sites + w * i, *row = s + w - 3;
            bool ok = row[0] >= 0 && row[1] >= 0;
            for (int k = 0; k < w - 3; k++) ok = ok && (s[k] == 0 || s[k] == 1);
            if (!ok) return fail(c, MP_ERR_ARG, "%s: site %lld is not {%s}", who, (long long)i, shape);
            if (row[0] >= (1 << 29)) return fail(c, MP_ERR_ARG, "%s: row %d of site %lld: at most 2^29 rows", who, row[0], (long long)i);
            if (i && !std::lexicographical_compare(s - w, s - 1, s, s + w - 1))
                return fail(c, MP_ERR_ARG, "%s: sites must ascend strictly in (%s) (site %lld)", who, order, (long long)i);
            max_row = std::max(max_row, row[0]);
        }
        n_rows = max_row + 1;
        n_bases = (long long)n_rows << 32;
        row_key.resize((size_t)n_rows);
        roff.resize((size_t)n_rows + 1);
        for (int r = 0; r <= n_rows; r++) roff[(size_t)r] = (int64_t)r << 32;
        for (int r = 0; r < n_rows; r++) row_key[(size_t)r] = r;
        int rc;
        if ((rc = d_rkey.alloc(row_key.size())) || (rc = d_roff.alloc(roff.size()))) return rc;
        return MP_OK;
    }
    hipError_t upload() {
        const hipError_t e = d_rkey.upload(row_key.data(), row_key.size());
        return e == hipSuccess ? d_roff.upload(roff.data(), roff.size()) : e;
    }
};

// what every entry of explicit sites starts with: they replace whatever the resident screen kept
void begin_explicit(mp_ctx *c, int64_t *n_out) {
    *n_out = 0;
    for (int i = 0; i < 4; i++) c->ot_ms[i] = 0;
    for (int i = 0; i < kOtCounts; i++) c->ot_counts[i] = 0;
    drop_products(c);
    c->ot_key.clear();
}

}  // namespace

extern "C" {

int mp_amplicon_join_classes(mp_ctx *c, int64_t n_sites, const int32_t *sites, int32_t size_lo, int32_t size_hi, int64_t cap, int32_t *out,
                             int64_t *n_out) {
    const char *who = "mp_amplicon_join_classes";
    if (!c) return MP_ERR_ARG;
    if (n_sites < 0 || !n_out || cap < 0 || (cap && !out) || (n_sites && !sites)) return fail(c, MP_ERR_ARG, "%s: bad arguments", who);
    HIPCK(c, hipSetDevice(c->dev));
    const auto t0 = std::chrono::steady_clock::now();
    begin_explicit(c, n_out);
    if (n_sites == 0) return MP_OK;
    SiteRows R(c);
    int rc;
    if ((rc = R.open(who, n_sites, sites, 5, "0|1, 0|1, row >= 0, pos >= 0, read", "class, strand, row, position"))) return rc;
    std::vector<long long> seg_key[4];
    std::vector<int32_t> seg_read[4];
    for (int64_t i = 0; i < n_sites; i++) {
        const int32_t *s = sites + 5 * i;
        seg_key[2 * s[0] + s[1]].push_back(((long long)s[2] << 32) + s[3]);
        seg_read[2 * s[0] + s[1]].push_back(s[4]);
    }
    DevBuf<long long> d_key(c);
    DevBuf<int32_t> d_primer(c);
    if ((rc = d_key.alloc((size_t)n_sites)) || (rc = d_primer.alloc((size_t)n_sites))) return rc;
    HIPCK_WAIT(c, R.upload());
    HIPCK(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> all;
    int64_t acc[kOtCounts] = {0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < kJoinClasses && rc == MP_OK; k++) {
        const auto &fk = seg_key[kJoinFwd[k]], &rk = seg_key[kJoinRev[k]];
        if (fk.empty() || rk.empty()) continue;
        std::vector<long long> key(fk);
        std::vector<int32_t> primer(seg_read[kJoinFwd[k]]);
        for (long long v : rk) key.push_back(R.n_bases + v);
        primer.insert(primer.end(), seg_read[kJoinRev[k]].begin(), seg_read[kJoinRev[k]].end());
        HIPCK_WAIT(c, d_key.upload(key.data(), key.size()));
        HIPCK_WAIT(c, d_primer.upload(primer.data(), primer.size()));
        HIPCK(c, hipStreamSynchronize(c->stream));          // (key and primer leave scope)
        rc = join_one_class(c, d_key.p, d_primer.p, (long long)key.size(), R.d_roff.p, R.n_rows, R.n_bases, R.d_rkey.p, size_lo, size_hi, k, all, acc);
    }
    (void)hipStreamSynchronize(c->stream);
    if (rc != MP_OK) return rc;
    for (int i = 0; i < kOtCounts; i++) c->ot_counts[i] = acc[i];
    rc = copy_out7(all, cap, out, n_out);
    c->ot_ms[2] = c->ot_ms[3] = ms_since(t0);
    return rc;
}

int mp_offtarget_classes(mp_ctx *c, int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off, const int32_t *read_id,
                         const int32_t *read_class, const int32_t *max_mm, int32_t term, int32_t size_lo, int32_t size_hi, int64_t cap,
                         int32_t *out, int64_t *n_out) {
    const char *who = "mp_offtarget_classes";
    if (!c) return MP_ERR_ARG;
    if (n_pat < 0 || !n_out || cap < 0 || (cap && !out) || (n_pat && (!pat_codes || !pat_off || !read_id || !read_class || !max_mm)) || term < 0)
        return fail(c, MP_ERR_ARG, "%s: bad arguments", who);
    HIPCK(c, hipSetDevice(c->dev));
    const auto t0 = std::chrono::steady_clock::now();
    *n_out = 0;
    for (int i = 0; i < 4; i++) c->ot_ms[i] = 0;
    int rc;
    if ((rc = kmm_check_patterns(c, n_pat, pat_codes, pat_off, [&](int32_t i) {
            if (max_mm[i] < 0) return fail(c, MP_ERR_ARG, "pattern %d has a negative mismatch budget", i);
            if (read_class[i] != 0 && read_class[i] != 1) return fail(c, MP_ERR_ARG, "pattern %d has class %d (0 core, 1 new)", i, read_class[i]);
            return (int)MP_OK;
        }))) return rc;
    // the six-column products of the plain screen do not survive this call (join_device reuses their buffer)
    drop_products(c);
    c->ot_key.clear();
    if (c->sq_n == 0 || n_pat == 0) {
        for (int i = 0; i < kOtCounts; i++) c->ot_counts[i] = 0;
        c->otc_out.clear();
        c->otc_key.clear();
        return MP_OK;
    }
    std::vector<uint8_t> key;
    const int32_t head[4] = {n_pat, term, size_lo, size_hi};
    put(key, head, 4);
    put(key, pat_off, (size_t)n_pat + 1);
    put(key, pat_codes + pat_off[0], (size_t)(pat_off[n_pat] - pat_off[0]));
    put(key, read_id, (size_t)n_pat);
    put(key, read_class, (size_t)n_pat);
    put(key, max_mm, (size_t)n_pat);
    if (!c->otc_key.empty() && key == c->otc_key) {         // a repeat of the last call: nothing is scanned again
        rc = copy_out7(c->otc_out, cap, out, n_out);
        c->ot_ms[3] = ms_since(t0);
        return rc;
    }
    c->otc_key.clear();
    c->otc_out.clear();
    for (int i = 0; i < kOtCounts; i++) c->ot_counts[i] = 0;
    const int n_rows = c->sq_n;
    std::vector<int32_t> row_key((size_t)n_rows);
    for (int r = 0; r < n_rows; r++) row_key[(size_t)r] = r;           // sequences in ascending store order
    Screen X(c, 4);
    DevBuf<int32_t> d_rid(c), d_rcls(c), d_rkey(c), jprimer(c);
    DevBuf<long long> d_bound(c), jkey(c);
    if ((rc = X.open(n_pat, pat_codes, pat_off, max_mm, -1, term)) || (rc = d_rid.alloc((size_t)n_pat)) || (rc = d_rcls.alloc((size_t)n_pat)) ||
        (rc = d_rkey.alloc((size_t)n_rows)) || (rc = d_bound.alloc(5))) return rc;
    if ((rc = X.clear())) return rc;
    HIPCK(c, d_rid.upload(read_id, (size_t)n_pat));
    HIPCK(c, d_rcls.upload(read_class, (size_t)n_pat));
    HIPCK(c, d_rkey.upload(row_key.data(), row_key.size()));
    HIPCK(c, hipStreamSynchronize(c->stream));              // (the stage times of this screen are host times: each stage ends in a wait)
    const auto t_scan = std::chrono::steady_clock::now();
    if ((rc = X.scan<0>(term, OtClassSites{X.map.p, c->sq_roff, X.n_bases, d_rcls.p, X.d_hits.p}))) return rc;
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->ot_ms[0] = ms_since(t_scan);
    const auto t_red = std::chrono::steady_clock::now();
    if ((rc = X.reduce(d_rid.p))) return rc;
    if ((rc = jkey.alloc(X.key.n)) || (rc = jprimer.alloc(X.key.n))) return rc;
    long long bound[5] = {0, 0, 0, 0, 0};
    hipLaunchKernelGGL(segment_bounds_kernel, dim3(1), dim3(64), 0, c->stream, (const long long *)X.key.p, X.n_sites, X.n_bases, d_bound.p);
    HIPCK_WAIT(c, hipGetLastError());
    HIPCK_WAIT(c, hipMemcpyAsync(bound, d_bound.p, sizeof bound, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->ot_ms[1] = ms_since(t_red);
    const auto t_join = std::chrono::steady_clock::now();
    std::vector<int32_t> all;
    int64_t acc[kOtCounts] = {0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < kJoinClasses && rc == MP_OK; k++) {
        const int fs = kJoinFwd[k], rs = kJoinRev[k];
        const long long n_f = bound[fs + 1] - bound[fs], n_r = bound[rs + 1] - bound[rs];
        if (n_f == 0 || n_r == 0) continue;
        hipLaunchKernelGGL(join_pick_kernel, dim3(grid(n_f + n_r, kBlock)), dim3(kBlock), 0, c->stream, (const long long *)X.key.p,
                           (const int32_t *)X.primer.p, bound[fs], n_f, (long long)fs * X.n_bases, bound[rs], n_r, (long long)rs * X.n_bases, X.n_bases,
                           jkey.p, jprimer.p);
        HIPCK_WAIT(c, hipGetLastError());
        rc = join_one_class(c, jkey.p, jprimer.p, n_f + n_r, c->sq_roff, n_rows, X.n_bases, d_rkey.p, size_lo, size_hi, k, all, acc);
    }
    (void)hipStreamSynchronize(c->stream);
    if (rc != MP_OK) return rc;
    c->ot_ms[2] = ms_since(t_join);
    acc[0] = (int64_t)X.hits;
    for (int i = 0; i < kOtCounts; i++) c->ot_counts[i] = acc[i];
    c->otc_out = std::move(all);
    c->otc_key = std::move(key);
    rc = copy_out7(c->otc_out, cap, out, n_out);
    c->ot_ms[3] = ms_since(t0);
    return rc;
}

int mp_offtarget_resident(mp_ctx *c, int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off, const int32_t *read_primer,
                          const int32_t *max_mm, int32_t term, int32_t size_lo, int32_t size_hi, int64_t cap, int32_t *out, int64_t *n_out) {
    return offtarget_run(c, "mp_offtarget_resident", n_pat, pat_codes, pat_off, read_primer, max_mm, -1, term, size_lo, size_hi, cap, out, n_out);
}

int mp_offtarget_gap_resident(mp_ctx *c, int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off, const int32_t *read_primer,
                              const int32_t *max_pen, int32_t max_gap, int32_t term, int32_t size_lo, int32_t size_hi, int64_t cap, int32_t *out,
                              int64_t *n_out) {
    if (c && max_gap < 0) return fail(c, MP_ERR_ARG, "mp_offtarget_gap_resident: max_gap %d (0..%d)", max_gap, MP_KMM_MAX_GAP);
    return offtarget_run(c, "mp_offtarget_gap_resident", n_pat, pat_codes, pat_off, read_primer, max_pen, max_gap, term, size_lo, size_hi, cap, out, n_out);
}

int mp_amplicon_join(mp_ctx *c, int64_t n_sites, const int32_t *sites, int32_t size_lo, int32_t size_hi, int64_t cap, int32_t *out, int64_t *n_out) {
    const char *who = "mp_amplicon_join";
    if (!c) return MP_ERR_ARG;
    if (n_sites < 0 || !n_out || cap < 0 || (cap && !out) || (n_sites && !sites)) return fail(c, MP_ERR_ARG, "%s: bad arguments", who);
    HIPCK(c, hipSetDevice(c->dev));
    const auto t0 = std::chrono::steady_clock::now();
    begin_explicit(c, n_out);
    if (n_sites == 0) return MP_OK;
    SiteRows R(c);
    int rc;
    if ((rc = R.open(who, n_sites, sites, 4, "0|1, row >= 0, pos >= 0, id", "strand, row, position"))) return rc;
    std::vector<long long> key((size_t)n_sites);
    std::vector<int32_t> primer((size_t)n_sites);
    for (int64_t i = 0; i < n_sites; i++) {
        const int32_t *s = sites + 4 * i;
        key[(size_t)i] = (s[0] ? R.n_bases : 0) + ((long long)s[1] << 32) + s[2];
        primer[(size_t)i] = s[3];
    }
    DevBuf<long long> d_key(c);
    DevBuf<int32_t> d_primer(c);
    if ((rc = d_key.alloc((size_t)n_sites)) || (rc = d_primer.alloc((size_t)n_sites))) return rc;
    HIPCK_WAIT(c, d_key.upload(key.data(), key.size()));
    HIPCK_WAIT(c, d_primer.upload(primer.data(), primer.size()));
    HIPCK_WAIT(c, R.upload());
    StageClock join;                         // the join alone, on the device's clock
    join.begin(c);
    rc = join_device(c, d_key.p, d_primer.p, n_sites, R.d_roff.p, R.n_rows, R.n_bases, R.d_rkey.p, size_lo, size_hi);
    if (rc == MP_OK) join.end(c);
    (void)hipStreamSynchronize(c->stream);               // (the host arrays above leave scope)
    join.read(c->ot_ms + 2);
    if (rc == MP_OK) rc = copy_out(c, cap, out, n_out);
    // what the join made stays only for this call's copy: it belongs to no store
    drop_products(c);
    c->ot_ms[3] = ms_since(t0);
    return rc;
}

int mp_offtarget_stats(mp_ctx *c, double *ms, int64_t *counts) {
    if (!c) return MP_ERR_ARG;
    for (int i = 0; i < 4; i++) if (ms) ms[i] = c->ot_ms[i];
    for (int i = 0; i < kOtCounts; i++) if (counts) counts[i] = c->ot_counts[i];
    return MP_OK;
}

}  // extern "C"
