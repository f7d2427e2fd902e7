// kmm.hpp — the k-mismatch primer-site scan kernel of scan.hip (mp_kmm_scan) and offtarget.hip (mp_offtarget_resident): one
// matching rule and one pattern table for both.  What a hit does is the Sink's business: scan.hip appends it to a hit list,
// offtarget.hip folds it into a per-position site map.
#pragma once

#include "common.hpp"

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
