// kmm.hpp — the k-mismatch primer-site scan: its kernels and the host code that drives them, one matching rule, one pattern table
// and one launch for its four users.  What a hit does is the Sink's business:
//   scan.hip       validation (mp_kmm_scan, mp_kmm_scan_resident, mp_kmm_gap_scan_resident): KmmAppend, every hit into a hit list
//   offtarget.hip  the off-target screen (mp_offtarget_resident, mp_offtarget_gap_resident): OtSites, a site map of two segments
//   offtarget.hip  the panel update's class screen (mp_offtarget_classes): OtClassSites, a site map of four segments
//   setscreen.hip  the set screen (mp_setscreen_add): SsAppend, de-duplicated site records into the screen's list
// The driver at the end of this file: kmm_check_patterns, KmmBlocks (the workgroups of a scan), kmm_table / kmm_tables, kmm_launch.
#pragma once

#include "common.hpp"
#include "../../include/mprime_offtarget.h"      // MP_KMM_MAX_GAP

namespace mp {
namespace {

constexpr int kSeg = 8192;                       // start positions per workgroup

// NW = 64-bit words of a pattern: 1 up to 32 bases, 2 up to MP_PATTERN_MAX_LEN = 64 (adaptor-tailed primers)
template <int NW>
struct KmmPat {
    unsigned long long word[NW];      // base j of the aligned text at bits 2 (j % 32) of word j / 32 (A0 C1 G2 T3)
    unsigned long long lenmask[NW];   // bit 2j set for j < len
    unsigned long long termmask[NW];  // bit 2j set for the last `term` positions in reference orientation (all of lenmask if term > len)
    int32_t len, id, strand, never;   // never: term > len — the trailing match run cannot reach the threshold
};

// RES: the text comes from the context's resident store (mp_seq_load: `code` / `flag` words at word offsets `woff`) — a segment is
// kSegWords coalesced 8-byte loads per plane instead of 32 byte loads and ~130 instructions per word
// Sink: `State begin()` per thread, `hit(state, row, p, pattern id, strand)` per accepted site, `end(state, row)` once per thread after its
// last position (every thread of the workgroup reaches it: no barrier inside).
template <int NW, bool RES, class Sink>
__global__ __launch_bounds__(kBlock) void kmm_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ row_off,
                                                     const unsigned long long *__restrict__ code, const unsigned long long *__restrict__ flag,
                                                     const int64_t *__restrict__ woff,
                                                     const int32_t *__restrict__ blk_row, const int32_t *__restrict__ blk_seg,
                                                     const KmmPat<NW> *__restrict__ pats, int n_pats, int max_mm, Sink sink) {
    constexpr int kSegWords = kSeg / 32 + 1 + NW;      // 64-bit words of 32 bases, with the overhang of the longest pattern
    __shared__ unsigned long long s_b[kSegWords];      // 2-bit codes
    __shared__ unsigned long long s_n[kSegWords];      // 0b01 at positions that match nothing (non-ACGT, past the end)
    const int row = blk_row[blockIdx.x], seg = blk_seg[blockIdx.x];
    const uint8_t *s = bytes + row_off[row];
    const long long len = row_off[row + 1] - row_off[row];
    const long long base = (long long)seg * kSeg;
    // pack: thread t builds word t (32 bases)
    for (int w = threadIdx.x; w < kSegWords; w += kBlock) {
        unsigned long long b = 0, n = 0;
        const long long p0 = base + (long long)w * 32;
        if (RES) {
            const long long gw = base / 32 + w, nwords = woff[row + 1] - woff[row];
            if (gw < nwords) { b = code[woff[row] + gw]; n = flag[woff[row] + gw] & 0x5555555555555555ull; }     // (the scan upper-cases: bit 2j alone)
            else n = 0x5555555555555555ull;
            s_b[w] = b; s_n[w] = n;
            continue;
        }
        for (int j = 0; j < 32; j++) {
            const long long p = p0 + j;
            unsigned long long code = 0, bad = 1;
            if (p < len) {
                uint8_t ch = s[p];
                if (ch >= 'a' && ch <= 'z') ch -= 32;
                if (ch == 'A') { code = 0; bad = 0; }
                else if (ch == 'C') { code = 1; bad = 0; }
                else if (ch == 'G') { code = 2; bad = 0; }
                else if (ch == 'T') { code = 3; bad = 0; }
            }
            b |= code << (2 * j);
            n |= bad << (2 * j);
        }
        s_b[w] = b;
        s_n[w] = n;
    }
    __syncthreads();
    const unsigned long long kOdd = 0x5555555555555555ull;
    auto st = sink.begin();
    for (int q = threadIdx.x; q < kSeg; q += kBlock) {
        const long long p = base + q;
        if (p >= len) break;
        const int w = q >> 5, sh = (q & 31) * 2;
        unsigned long long win[NW], nw[NW];
#pragma unroll
        for (int t = 0; t < NW; t++) {
            win[t] = s_b[w + t] >> sh; nw[t] = s_n[w + t] >> sh;
            if (sh) { win[t] |= s_b[w + t + 1] << (64 - sh); nw[t] |= s_n[w + t + 1] << (64 - sh); }
        }
        for (int i = 0; i < n_pats; i++) {
            const KmmPat<NW> P = pats[i];               // uniform index: scalar loads
            int n_mm = 0;
            unsigned long long in_term = 0;
#pragma unroll
            for (int t = 0; t < NW; t++) {
                const unsigned long long x = win[t] ^ P.word[t];
                const unsigned long long mm = (((x | (x >> 1)) & kOdd) | nw[t]) & P.lenmask[t];
                n_mm += (int)__popcll(mm);
                in_term |= mm & P.termmask[t];
            }
            if (n_mm <= max_mm && in_term == 0 && !P.never && p + P.len <= len) sink.hit(st, row, p, P.id, P.strand);
        }
    }
    sink.end(st, row);
}

// ---- the gapped form (include/mprime_offtarget.h: mp_kmm_gap_scan_resident, mp_offtarget_gap_resident) -----------------------------
// bowtie2's end-to-end rule with at most ONE gap of g <= MP_KMM_MAX_GAP bases beside the mismatches: a site is a hit when the ungapped
// rule holds with pen / 6 mismatches (kmm_kernel's test), or when, for some g with 5 + 3 g <= pen and some split column c,
//   type D  read base j pairs with T[p + j] below c and with T[p + g + j] from c on   (kGbar <= c <= L - kGbar, p + L + g <= len)
//   type I  read base j pairs with T[p + j] below c, bases c .. c + g - 1 pair with nothing, base j >= c + g pairs with T[p + j - g]
//           (kGbar <= c, c + g <= L - kGbar, p + L - g <= len)
// has 6 mm + 5 + 3 g <= pen and its last `term` aligned pairs match (type D: all of them right of the deletion).
// Both types read the same way in TEXT columns k (the offset from p of the text base a pair uses, less g right of a deletion): columns
// below c come from the diagonal-0 mismatch mask A, columns from c on from a shifted mask B — the text moved by g (type D), or the
// PATTERN moved by g and cut to L - g columns (type I: nothing left of p is read).  So no loop over c: with m = (pen - 5 - 3 g) / 6,
// |A below c| <= i  <=>  c <= the (i + 1)-th lowest set bit of A, and |B from c| <= m - i  <=>  c > the (m - i + 1)-th highest set bit
// of B; for i = 0 .. m these bound an interval of c, cut by the kGbar bounds and the 3' term (type D: c <= L - term and no set bit of
// B in the term columns; type I: c above B's highest and at most A's lowest set bit in the term columns L - g - term .. L - g - 1), and
// the alignment exists iff one of the m + 1 intervals is not empty.  Masks keep kmm_kernel's layout (column k at bit 2k), so every
// bound below is a BIT index, twice the column.
constexpr int kGbar = MP_KMM_GBAR;                      // bowtie2 --gbar: no gap within this many bases of either read end

template <int NW> __device__ inline int kmm_pop(const unsigned long long (&x)[NW]) {
    int n = 0;
#pragma unroll
    for (int t = 0; t < NW; t++) n += (int)__popcll(x[t]);
    return n;
}
template <int NW> __device__ inline int kmm_low(const unsigned long long (&x)[NW]) {      // lowest set bit; 64 NW: none
    int r = 64 * NW;
#pragma unroll
    for (int t = NW - 1; t >= 0; t--) if (x[t]) r = 64 * t + __ffsll((long long)x[t]) - 1;
    return r;
}
template <int NW> __device__ inline int kmm_high(const unsigned long long (&x)[NW]) {     // highest set bit; -2: none (one column below 0)
    int r = -2;
#pragma unroll
    for (int t = 0; t < NW; t++) if (x[t]) r = 64 * t + 63 - __clzll((long long)x[t]);
    return r;
}
template <int NW> __device__ inline void kmm_drop_low(unsigned long long (&x)[NW]) {
    bool done = false;
#pragma unroll
    for (int t = 0; t < NW; t++) if (!done && x[t]) { x[t] &= x[t] - 1; done = true; }
}
template <int NW> __device__ inline void kmm_drop_high(unsigned long long (&x)[NW]) {
    bool done = false;
#pragma unroll
    for (int t = NW - 1; t >= 0; t--) if (!done && x[t]) { x[t] &= ~(1ull << (63 - __clzll((long long)x[t]))); done = true; }
}
// x >> s across words (0 < s < 64; zeros come in at the top)
template <int NW> __device__ inline void kmm_shr(const unsigned long long (&x)[NW], int s, unsigned long long (&y)[NW]) {
#pragma unroll
    for (int t = 0; t < NW; t++) y[t] = (x[t] >> s) | (t + 1 < NW ? x[t + 1] << (64 - s) : 0ull);
}

// a split bit c in [lo, hi] with |A below c| + |B from c| <= m ?
template <int NW>
__device__ inline bool kmm_gap_split(const unsigned long long (&A)[NW], const unsigned long long (&B)[NW], int m, int lo, int hi) {
    if (lo > hi) return false;
    unsigned long long a[NW], bh[NW];
#pragma unroll
    for (int t = 0; t < NW; t++) { a[t] = A[t]; bh[t] = B[t]; }
    int removed = 0;                                   // B's highest set bits taken out of bh: min(m - i, |B|)
    for (; removed < m && kmm_high<NW>(bh) >= 0; removed++) kmm_drop_high<NW>(bh);
    for (int i = 0;; i++) {
        if (max(kmm_high<NW>(bh) + 2, lo) <= min(kmm_low<NW>(a), hi)) return true;
        if (i == m) return false;
        kmm_drop_low<NW>(a);
        if (removed > m - i - 1) {                     // the lowest of the removed bits comes back
            unsigned long long out[NW];
#pragma unroll
            for (int t = 0; t < NW; t++) out[t] = B[t] & ~bh[t];
            const int b = kmm_low<NW>(out);
#pragma unroll
            for (int t = 0; t < NW; t++) if (b >> 6 == t) bh[t] |= 1ull << (b & 63);
            removed--;
        }
    }
}

// Resident store only.  The window of a start is NW + 1 words (L + MP_KMM_MAX_GAP bases), so a segment's overhang is one word more than
// kmm_kernel's.  `pen`: the penalty ceiling; `max_gap` >= 1; `term` as the pattern table was built with.
template <int NW, class Sink>
__global__ __launch_bounds__(kBlock) void kmm_gap_kernel(const int64_t *__restrict__ row_off, const unsigned long long *__restrict__ code,
                                                         const unsigned long long *__restrict__ flag, const int64_t *__restrict__ woff,
                                                         const int32_t *__restrict__ blk_row, const int32_t *__restrict__ blk_seg,
                                                         const KmmPat<NW> *__restrict__ pats, int n_pats, int pen, int max_gap, int term, Sink sink) {
    constexpr int kSegWords = kSeg / 32 + 2 + NW;      // the window of the last start reads words w .. w + NW + 1
    __shared__ unsigned long long s_b[kSegWords];
    __shared__ unsigned long long s_n[kSegWords];
    const unsigned long long kOdd = 0x5555555555555555ull;
    const int row = blk_row[blockIdx.x], seg = blk_seg[blockIdx.x];
    const long long len = row_off[row + 1] - row_off[row];
    const long long base = (long long)seg * kSeg;
    const long long nwords = woff[row + 1] - woff[row];
    for (int w = threadIdx.x; w < kSegWords; w += kBlock) {
        const long long gw = base / 32 + w;
        unsigned long long b = 0, n = kOdd;
        if (gw < nwords) { b = code[woff[row] + gw]; n = flag[woff[row] + gw] & kOdd; }
        s_b[w] = b; s_n[w] = n;
    }
    __syncthreads();
    const int max_mm = pen / 6;
    const int n_g = min(min(max_gap, MP_KMM_MAX_GAP), pen >= 5 ? (pen - 5) / 3 : 0);     // gap lengths the ceiling admits
    const int m1 = pen >= 8 ? (pen - 8) / 6 : 0;                                        // mismatches beside a 1-base gap: the most
    auto st = sink.begin();
    for (int q = threadIdx.x; q < kSeg; q += kBlock) {
        const long long p = base + q;
        if (p >= len) break;
        const int w = q >> 5, sh = (q & 31) * 2;
        unsigned long long win[NW + 1], nw[NW + 1];
#pragma unroll
        for (int t = 0; t <= NW; t++) {
            win[t] = s_b[w + t] >> sh; nw[t] = s_n[w + t] >> sh;
            if (sh) { win[t] |= s_b[w + t + 1] << (64 - sh); nw[t] |= s_n[w + t + 1] << (64 - sh); }
        }
        for (int i = 0; i < n_pats; i++) {
            const KmmPat<NW> P = pats[i];               // uniform index: scalar loads
            if (P.never) continue;
            const int L = P.len;
            unsigned long long A[NW], in_term = 0;
#pragma unroll
            for (int t = 0; t < NW; t++) {
                const unsigned long long x = win[t] ^ P.word[t];
                A[t] = (((x | (x >> 1)) & kOdd) | nw[t]) & P.lenmask[t];
                in_term |= A[t] & P.termmask[t];
            }
            bool hit = kmm_pop<NW>(A) <= max_mm && in_term == 0 && p + L <= len;
            // every gapped alignment keeps columns 0 .. kGbar - 1 on diagonal 0: more than m1 mismatches there end it
            const int head = (int)__popcll(A[0] & ((1ull << (2 * kGbar)) - 1));
            if (!hit && n_g > 0 && head <= m1) {
                unsigned long long tail[NW];            // the last kGbar columns of L: always right of a deletion
                kmm_shr<NW>(P.lenmask, 2 * kGbar, tail);
#pragma unroll
                for (int t = 0; t < NW; t++) tail[t] = P.lenmask[t] & ~tail[t];
#pragma unroll
                for (int g = 1; g <= MP_KMM_MAX_GAP; g++) {
                    const int m = (pen - 5 - 3 * g) / 6;
                    if (g > n_g || hit || head > m) break;
                    unsigned long long B[NW], TB[NW], TA[NW];
                    // type D: the text g bases on
                    if (p + L + g <= len && L >= 2 * kGbar) {
                        unsigned long long tb = 0;
                        int last = 0;
#pragma unroll
                        for (int t = 0; t < NW; t++) {
                            const unsigned long long tx = (win[t] >> (2 * g)) | (win[t + 1] << (64 - 2 * g));
                            const unsigned long long tn = (nw[t] >> (2 * g)) | (nw[t + 1] << (64 - 2 * g));
                            const unsigned long long x = tx ^ P.word[t];
                            B[t] = (((x | (x >> 1)) & kOdd) | tn) & P.lenmask[t];
                            tb |= B[t] & P.termmask[t];
                            last += (int)__popcll(B[t] & tail[t]);
                        }
                        if (tb == 0 && last <= m) hit = kmm_gap_split<NW>(A, B, m, 2 * kGbar, 2 * min(L - kGbar, L - term));
                    }
                    // type I: the pattern g bases on, L - g columns
                    if (!hit && p + L - g <= len && L - g >= 2 * kGbar && term <= L - g) {
                        unsigned long long pw[NW], pl[NW], pt[NW];
                        kmm_shr<NW>(P.word, 2 * g, pw);
                        kmm_shr<NW>(P.lenmask, 2 * g, pl);
                        kmm_shr<NW>(P.termmask, 2 * g, pt);
#pragma unroll
                        for (int t = 0; t < NW; t++) {
                            const unsigned long long x = win[t] ^ pw[t];
                            B[t] = (((x | (x >> 1)) & kOdd) | nw[t]) & pl[t];
                            TB[t] = B[t] & pt[t];
                            TA[t] = A[t] & pt[t];
                        }
                        hit = kmm_gap_split<NW>(A, B, m, max(2 * kGbar, kmm_high<NW>(TB) + 2), min(2 * (L - g - kGbar), kmm_low<NW>(TA)));
                    }
                }
            }
            if (hit) sink.hit(st, row, p, P.id, P.strand);
        }
    }
    sink.end(st, row);
}

// mp_kmm_scan's sink: every hit appended to one list of {sequence, p, pattern, strand}; past `cap` only counted
struct KmmAppend {
    struct State {};
    long long cap;
    int32_t *hits;
    unsigned long long *n_hits;
    __device__ State begin() const { return {}; }
    __device__ void hit(State &, int row, long long p, int id, int strand) const {
        const unsigned long long idx = atomicAdd(n_hits, 1ull);
        if ((long long)idx < cap) {
            hits[4 * idx] = row; hits[4 * idx + 1] = (int32_t)p; hits[4 * idx + 2] = id; hits[4 * idx + 3] = strand;
        }
    }
    __device__ void end(State &, int) const {}
};

// both strands of every pattern as kernel table entries
template <int NW>
void kmm_patterns(int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off, int32_t term, std::vector<KmmPat<NW>> &pats) {
    for (int32_t i = 0; i < n_pat; i++) {
        const int len = pat_off[i + 1] - pat_off[i];
        int b[MP_PATTERN_MAX_LEN];
        for (int j = 0; j < len; j++) {
            const uint8_t m = pat_codes[pat_off[i] + j];
            b[j] = m == 1 ? 0 : m == 2 ? 1 : m == 4 ? 2 : 3;
        }
        for (int strand = 0; strand < 2; strand++) {
            KmmPat<NW> P{};
            for (int j = 0; j < len; j++) {
                const int code = strand == 0 ? b[j] : 3 - b[len - 1 - j];      // the text reads the pattern / its reverse complement
                P.word[j >> 5] |= (unsigned long long)code << (2 * (j & 31));
                P.lenmask[j >> 5] |= 1ull << (2 * (j & 31));
                if (j >= len - term) P.termmask[j >> 5] |= 1ull << (2 * (j & 31));
            }
            P.len = len; P.id = i; P.strand = strand; P.never = term > len;
            pats.push_back(P);
        }
    }
}

// ---- the driver: what every scan does on the host ------------------------------------------------------------------------------------
// the one pattern check: a length the tables hold, concrete bases only; then `also(i)`, what the caller asks of pattern i beside that
// (patterns are checked in order, so the first pattern at fault is the one reported)
template <class Also>
int kmm_check_patterns(mp_ctx *c, int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off, Also also) {
    for (int32_t i = 0; i < n_pat; i++) {
        const int len = pat_off[i + 1] - pat_off[i];
        if (len < 4 || len > MP_PATTERN_MAX_LEN) return fail(c, MP_ERR_ARG, "pattern %d has length %d (4..%d supported)", i, len, MP_PATTERN_MAX_LEN);
        for (int j = 0; j < len; j++) {
            const uint8_t m = pat_codes[pat_off[i] + j];
            if (m != 1 && m != 2 && m != 4 && m != 8) return fail(c, MP_ERR_ARG, "pattern %d is not a concrete A/C/G/T sequence", i);
        }
        if (int rc = also(i)) return rc;
    }
    return MP_OK;
}
inline int kmm_check_patterns(mp_ctx *c, int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off) {
    return kmm_check_patterns(c, n_pat, pat_codes, pat_off, [](int32_t) { return MP_OK; });
}

// The workgroups of a scan: one per (record, segment of kSeg starts), built on the host per call and uploaded.  The host lists live as
// long as the object: upload() is covered by the next synchronisation of the stream, which comes before the object goes.
struct KmmBlocks {
    std::vector<int32_t> row, seg;
    DevBuf<int32_t> d_row, d_seg;
    size_t n = 0;
    explicit KmmBlocks(mp_ctx *c) : d_row(c), d_seg(c) {}
    size_t size() const { return n; }
    void drop_host() { std::vector<int32_t>().swap(row); std::vector<int32_t>().swap(seg); }      // after the wait that covers upload()
    int build(const int64_t *roff_host, int32_t n_rows) {
        for (int32_t r = 0; r < n_rows; r++) {
            const int64_t len = roff_host[r + 1] - roff_host[r];
            if (len < 0 || len > 0x7fffffffLL) return fail(d_row.c, MP_ERR_ARG, "sequence %d has bad length", r);
            for (int64_t sgm = 0; sgm * kSeg < len; sgm++) { row.push_back(r); seg.push_back((int32_t)sgm); }
        }
        n = row.size();
        int rc;
        if ((rc = d_row.alloc(n)) || (rc = d_seg.alloc(n))) return rc;
        return MP_OK;
    }
    hipError_t upload() {
        const hipError_t e = d_row.upload(row.data(), row.size());
        return e == hipSuccess ? d_seg.upload(seg.data(), seg.size()) : e;
    }
    void release() { d_row.release(); d_seg.release(); }
};

// One launch's pattern table: `n` entries of KmmPat<two ? 2 : 1> in `bytes`.  gaps > 0: kmm_gap_kernel with the penalty ceiling `budget`
// and gaps of up to `gaps` bases; else kmm_kernel with `budget` mismatches.
struct KmmTable { int32_t budget; bool two; std::vector<uint8_t> bytes; int n; int32_t gaps; };

// the table of the patterns idx[] in that order, both strands each; an entry's id is id_of[i] (null: i) of its pattern i; two words
// per pattern as soon as one of them has more than 32 bases
inline KmmTable kmm_table(const std::vector<int32_t> &idx, const uint8_t *pat_codes, const int32_t *pat_off, const int32_t *id_of, int32_t term) {
    std::vector<uint8_t> codes;
    std::vector<int32_t> off{0};
    int longest = 0;
    for (int32_t i : idx) {
        codes.insert(codes.end(), pat_codes + pat_off[i], pat_codes + pat_off[i + 1]);
        off.push_back((int32_t)codes.size());
        longest = std::max(longest, pat_off[i + 1] - pat_off[i]);
    }
    KmmTable T{0, longest > 32, {}, 0, 0};
    auto fill = [&](auto &pats) {
        kmm_patterns((int32_t)idx.size(), codes.data(), off.data(), term, pats);
        for (auto &P : pats) P.id = id_of ? id_of[idx[(size_t)P.id]] : idx[(size_t)P.id];
        T.n = (int)pats.size();
        put(T.bytes, pats.data(), pats.size());
    };
    if (T.two) { std::vector<KmmPat<2>> p; fill(p); } else { std::vector<KmmPat<1>> p; fill(p); }
    return T;
}

// The table's rule.  max_gap < 0: b is a mismatch budget; max_gap >= 0: a penalty ceiling under the gapped rule — a table whose ceiling
// admits a gap (5 + 3 g <= ceiling, g <= max_gap) goes through kmm_gap_kernel, the others through kmm_kernel with ceiling / 6
// mismatches: the same sites.
inline KmmTable kmm_budget(KmmTable T, int32_t b, int32_t max_gap) {
    T.gaps = max_gap > 0 && b >= 8 ? std::min<int32_t>(max_gap, (b - 5) / 3) : 0;
    T.budget = max_gap >= 0 && T.gaps == 0 ? b / 6 : b;
    return T;
}

// one table per distinct budget[i], ascending (ids: the pattern's index), each under kmm_budget's rule
inline std::vector<KmmTable> kmm_tables(int32_t n_pat, const uint8_t *pat_codes, const int32_t *pat_off, const int32_t *budget, int32_t max_gap,
                                        int32_t term) {
    std::vector<int32_t> budgets(budget, budget + n_pat);
    std::sort(budgets.begin(), budgets.end());
    budgets.erase(std::unique(budgets.begin(), budgets.end()), budgets.end());
    std::vector<KmmTable> tables;
    for (int32_t b : budgets) {
        std::vector<int32_t> idx;
        for (int32_t i = 0; i < n_pat; i++) if (budget[i] == b) idx.push_back(i);
        tables.push_back(kmm_budget(kmm_table(idx, pat_codes, pat_off, nullptr, term), b, max_gap));
    }
    return tables;
}

inline size_t kmm_table_bytes(const std::vector<KmmTable> &tables) {      // room for the largest of them
    size_t n = 1;
    for (auto &T : tables) n = std::max(n, T.bytes.size());
    return n;
}

// the text of a scan: the context's resident store, or (code == null) the bytes of the call
struct KmmText {
    const uint8_t *bytes;
    const int64_t *roff;
    const unsigned long long *code, *flag;
    const int64_t *woff;
};
inline KmmText kmm_store(const mp_ctx *c) { return {c->sq_bytes, c->sq_roff, c->sq_code, c->sq_flag, c->sq_woff}; }

// what a caller's launches may need beside kmm_kernel on the store (no kernel is compiled for a form its caller never takes)
constexpr int kKmmBytes = 1;                     // the text may be the bytes of the call
constexpr int kKmmGaps = 2;                      // a table may admit gaps

template <int NW, int FORMS, class Sink>
void kmm_launch_words(mp_ctx *c, const KmmText &X, const KmmBlocks &B, const KmmTable &T, const uint8_t *d_pats, int32_t term, const Sink &sink) {
    const dim3 g((unsigned)B.size()), b(kBlock);
    const KmmPat<NW> *pats = reinterpret_cast<const KmmPat<NW> *>(d_pats);
    const int32_t *brow = B.d_row.p, *bseg = B.d_seg.p;
    if constexpr ((FORMS & kKmmGaps) != 0) {
        if (T.gaps > 0) {
            hipLaunchKernelGGL((kmm_gap_kernel<NW, Sink>), g, b, 0, c->stream, X.roff, X.code, X.flag, X.woff, brow, bseg, pats, T.n, (int)T.budget,
                               (int)T.gaps, (int)term, sink);
            return;
        }
    }
    if constexpr ((FORMS & kKmmBytes) != 0) {
        if (!X.code) {
            hipLaunchKernelGGL((kmm_kernel<NW, false, Sink>), g, b, 0, c->stream, X.bytes, X.roff, X.code, X.flag, X.woff, brow, bseg, pats, T.n,
                               (int)T.budget, sink);
            return;
        }
    }
    hipLaunchKernelGGL((kmm_kernel<NW, true, Sink>), g, b, 0, c->stream, X.bytes, X.roff, X.code, X.flag, X.woff, brow, bseg, pats, T.n, (int)T.budget, sink);
}

// One launch: table T (already at d_pats) over the workgroups B of text X into `sink`.  B.size() > 0.
template <int FORMS, class Sink>
hipError_t kmm_launch(mp_ctx *c, const KmmText &X, const KmmBlocks &B, const KmmTable &T, const uint8_t *d_pats, int32_t term, const Sink &sink) {
    if (T.two) kmm_launch_words<2, FORMS>(c, X, B, T, d_pats, term, sink);
    else kmm_launch_words<1, FORMS>(c, X, B, T, d_pats, term, sink);
    return hipGetLastError();
}

}  // namespace
}  // namespace mp
