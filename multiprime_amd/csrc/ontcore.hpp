// ontcore.hpp — the match count of include/mprime_ont.h on position masks: what a lane of ont_assign_kernel (ont.hip) runs for one
// (piece, key) pair.  W is the mask word: uint64_t for strings of up to 64 bytes, uint32_t when piece and key have at most 32 (the usual
// 18 .. 22 bases: every shift is then one 32-bit instruction).  Plain integer C++, host and device, so that a CPU build can run the very
// same routine (tools/ont_emul.cpp).
#pragma once

#include <stdint.h>

#include "../../include/mprime_ont.h"

#if defined(__HIPCC__)
#define MP_ONT_HD __host__ __device__ __forceinline__
#else
#define MP_ONT_HD inline
#endif

namespace mp {

// entries of the range stack: a chain of t nested matches leaves at most t + 1 pending ranges and uses 2 t + 1 letters of the piece
template <typename W> constexpr int ont_stack_entries() { return sizeof(W) == 8 ? MP_ONT_STACK : MP_ONT_STACK / 2 + 1; }

MP_ONT_HD int ont_min(int a, int b) { return a < b ? a : b; }
MP_ONT_HD int ont_max(int a, int b) { return a > b ? a : b; }

MP_ONT_HD int ont_popc(uint64_t x) { return __builtin_popcountll(x); }
MP_ONT_HD int ont_popc(uint32_t x) { return __builtin_popcount(x); }
MP_ONT_HD int ont_ctz(uint64_t x) { return __builtin_ctzll(x); }
MP_ONT_HD int ont_ctz(uint32_t x) { return __builtin_ctz(x); }

MP_ONT_HD int ont_code(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4; }

// a range of the pair: four numbers of 0 .. 64
MP_ONT_HD uint32_t pack_range(int alo, int ahi, int blo, int bhi) {
    return (uint32_t)alo | ((uint32_t)ahi << 8) | ((uint32_t)blo << 16) | ((uint32_t)bhi << 24);
}

// One diagonal d = j - i of the range: x has bit i set where a[i] == b[i + d], i and i + d inside the range.  The longest run of ones,
// lowest start first, replaces (bk, bi, bd) if it is longer, or as long and starts earlier in a.  Diagonals are walked in ascending d,
// so among equal (k, i) the smaller j = i + d stays.
template <typename W, bool NEG>
MP_ONT_HD void ont_diagonal(const W (&pa)[4], const W (&kb)[4], int d, int alo, int ahi, int blo, int bhi, int &bk, int &bi, int &bd) {
    constexpr int B = 8 * (int)sizeof(W);
    const int s = NEG ? -d : d;                // 0 .. B - 1
    W x;
    if (NEG) x = (pa[0] & (kb[0] << s)) | (pa[1] & (kb[1] << s)) | (pa[2] & (kb[2] << s)) | (pa[3] & (kb[3] << s));
    else x = (pa[0] & (kb[0] >> s)) | (pa[1] & (kb[1] >> s)) | (pa[2] & (kb[2] >> s)) | (pa[3] & (kb[3] >> s));
    const int ilo = ont_max(alo, blo - d), ihi = ont_min(ahi, bhi - d);       // 0 <= ilo < ihi <= B for every d of the range
    x &= ((W)~(W)0 >> (B - ihi)) & ((W)~(W)0 << ilo);
    if (ont_popc(x) < ont_max(bk, 1)) return;      // fewer ones than the run to beat
    int k = 0;
    W y;
    do { y = x; x &= (W)(x >> 1); k++; } while (x);
    const int i = ont_ctz(y);
    if (k > bk || (k == bk && i < bi)) { bk = k; bi = i; bd = d; }
}

// M(a, b) of mprime_ont.h; la and lb at most the bits of W.  stk: the lane's LDS column, entry e at stk[e * stride] (an LDS column per lane on the device).
template <typename W>
MP_ONT_HD int ont_matches(const W (&pa)[4], int la, const W (&kb)[4], int lb, uint32_t *stk, int stride) {
    if (la == 0 || lb == 0) return 0;
    int M = 0, sp = 0;
    uint32_t cur = pack_range(0, la, 0, lb);
    for (;;) {
        const int alo = (int)(cur & 0xFF), ahi = (int)((cur >> 8) & 0xFF), blo = (int)((cur >> 16) & 0xFF), bhi = (int)(cur >> 24);
        int bk = 0, bi = 0, bd = 0;
        const int dlo = blo - (ahi - 1), dhi = (bhi - 1) - alo;
        for (int d = dlo; d <= ont_min(dhi, -1); d++) ont_diagonal<W, true>(pa, kb, d, alo, ahi, blo, bhi, bk, bi, bd);
        for (int d = ont_max(dlo, 0); d <= dhi; d++) ont_diagonal<W, false>(pa, kb, d, alo, ahi, blo, bhi, bk, bi, bd);
        bool have = false;
        if (bk) {
            M += bk;
            const int bj = bi + bd;
            const bool left = alo < bi && blo < bj, right = bi + bk < ahi && bj + bk < bhi;
            if (left && right && sp < ont_stack_entries<W>()) stk[sp++ * stride] = pack_range(alo, bi, blo, bj);
            if (right) { cur = pack_range(bi + bk, ahi, bj + bk, bhi); have = true; }
            else if (left) { cur = pack_range(alo, bi, blo, bj); have = true; }
        }
        if (!have) {
            if (sp == 0) break;
            cur = stk[--sp * stride];
        }
    }
    return M;
}

// four position masks and the length of a string of at most 64 bytes; a byte that is none of A, C, G, T is in no mask
MP_ONT_HD void ont_masks(const uint8_t *b, int len, uint64_t m[4]) {
    m[0] = m[1] = m[2] = m[3] = 0;
    for (int i = 0; i < len; i++) {
        const int cd = ont_code(b[i]);
        if (cd < 4) m[cd] |= 1ull << i;
    }
}

}  // namespace mp
