// kmm.hpp — the k-mismatch primer-site scan kernel of scan.hip (mp_kmm_scan) and offtarget.hip (mp_offtarget_resident): one
// matching rule and one pattern table for both.  What a hit does is the Sink's business: scan.hip appends it to a hit list,
// offtarget.hip folds it into a per-position site map.
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

}  // namespace
}  // namespace mp
