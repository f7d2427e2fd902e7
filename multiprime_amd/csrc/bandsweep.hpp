// bandsweep.hpp — the banded affine-gap (Gotoh) sweep around a voted seed diagonal, the one rule behind anchored alignment, the star
// alignment (anchorcore.hpp: anchor_dp_kernel) and clustering by identity (cluster.hip: cluster_dp_kernel).  One wavefront per alignment,
// lanes own the band's diagonals: R = 1, 2, 4 or 8 neighbouring diagonals per lane for 2W + 1 <= 64 R.  ANTI-DIAGONAL sweep: at step s
// the cells with i + j = s are computed; cell (i, j) on diagonal d reads its left cell (i, j-1) from diagonal d - 1 and its upper cell
// (i-1, j) from diagonal d + 1, both computed at step s - 1, and its diagonal cell from its own registers — no dependency inside a step,
// so no scan; a lane is busy every other step.  The pair score is two compares on the letters' codes.
// band_sweep decides; what is kept of a decision is the caller's PAYLOAD (the traceback bits of anchorcore.hpp, the carried counts of
// cluster.hip), which the sweep calls:
//   start(r, on_edge)        once per diagonal slot r of the lane, before the first step
//   exchange()               once per step, all lanes: the payload's own exchange of its edge slots with the neighbouring lanes
//   outside(r, t, i)         the cell of row i on band diagonal t lies outside the matrix
//   cell(r, t, i, j, on_edge, h_source, e_opened, f_opened, is_match)
//                            the cell (i, j): H came from h_source (kFromDiag, kFromE, kFromF), E and F were opened here (from H) or
//                            extended, the diagonal move pairs two equal letters; on_edge: t is the band's first or last diagonal.
//                            The slots r - 1 and r + 1 (or the exchanged edges) still hold the step before: a step's cells have one parity
//   joined(r, t, i)          after either of the two, where the sweep writes the cell's own H, E and F: the one place per slot for what
//                            a payload does for every cell alike
//   finish(lane, r)          all lanes, only where a path exists: the end cell is slot r of `lane`
// Everything sits in an unnamed namespace and nothing here is a kernel: a translation unit gets the kernels it defines itself.
#pragma once

#include "common.hpp"
#include "../../include/mprime_anchor.h"

#include <type_traits>

namespace mp {

namespace {

constexpr int kNeg = -(1 << 30);               // "no such cell": below every real score by more than any real score can gain
constexpr int kNoPath = -(3 << 28);            // a best end score below this was never fed by row 0 (mprime_anchor.h: MP_ANCHOR_MAX_PARAM)
constexpr int kWord = MP_ANCHOR_WORD;

enum : int { kFromDiag = 0, kFromE = 1, kFromF = 2 };

// diagonals per lane of the sweep for a band of half width W: 2W + 1 <= 64 R
inline int lane_diagonals(int W) { const int B = 2 * W + 1; return B <= 64 ? 1 : B <= 128 ? 2 : B <= 256 ? 4 : 8; }

// f(std::integral_constant<int, R>) for R = lane_diagonals(W): the launch of a kernel template over R
template <class F>
inline void for_lane_diagonals(int W, F &&f) {
    switch (lane_diagonals(W)) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: f(std::integral_constant<int, 8>{}); break;
    }
}

// the end cell: the largest H(m, j) of the band, the smallest j (= the smallest band diagonal t) among equals; no path: MP_ANCHOR_NO_SCORE, -1
struct BandEnd { int score, t; };

// The sweep of one wavefront: query codes qc[0 .. m) and anchor codes ac[0 .. n) in LDS, band diagonals dlo .. dlo + 2W (t = 0 .. 2W,
// lane l owns t = l R .. l R + R - 1).  Every lane returns the same BandEnd.
template <int R, class Payload>
__device__ __forceinline__ BandEnd band_sweep(const uint8_t *qc, const uint8_t *ac, int m, int n, int dlo, int W, int match, int mismatch, int open_ext,
                                              int ext, Payload &pay) {
    const int lane = threadIdx.x & 63, B = 2 * W + 1;
    int H[R], E[R], F[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int t = lane * R + r, d = dlo + t;
        H[r] = (t < B && d >= 0 && d <= n) ? 0 : kNeg;          // the row-0 cell of the diagonal
        E[r] = F[r] = kNeg;
        pay.start(r, t == 0 || t == B - 1);
    }
    const int s_end = 2 * m + dlo + B - 1;
    for (int s = 2 + dlo; s <= s_end; s++) {
        // the neighbouring lanes' edge diagonals as of step s - 1
        int hl_edge = __shfl_up(H[R - 1], 1), el_edge = __shfl_up(E[R - 1], 1);
        int hu_edge = __shfl_down(H[0], 1), fu_edge = __shfl_down(F[0], 1);
        pay.exchange();
        if (lane == 0) hl_edge = el_edge = kNeg;
        if (lane == 63) hu_edge = fu_edge = kNeg;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int t = lane * R + r, d = dlo + t, two_i = s - d;
            if ((two_i & 1) || two_i < 2 || two_i > 2 * m || t >= B) continue;       // (the cells of one step have one parity: H[r +- 1] are of step s - 1)
            const int i = two_i >> 1, j = i + d;
            int h = kNeg, e = kNeg, f = kNeg;
            if (j >= 0 && j <= n) {
                const int hl = r > 0 ? H[r > 0 ? r - 1 : 0] : hl_edge, el = r > 0 ? E[r > 0 ? r - 1 : 0] : el_edge;
                const int hu = r < R - 1 ? H[r < R - 1 ? r + 1 : 0] : hu_edge, fu = r < R - 1 ? F[r < R - 1 ? r + 1 : 0] : fu_edge;
                const int eo = hl - open_ext, ee = el - ext, fo = hu - open_ext, fe = fu - ext;
                e = max(eo, ee);
                f = max(fo, fe);
                int dg = kNeg;
                bool is_match = false;
                if (j >= 1) {
                    const int qcd = qc[i - 1], acd = ac[j - 1];
                    const bool both = qcd < 4 && acd < 4;
                    dg = H[r] + (both ? (qcd == acd ? match : -mismatch) : 0);
                    is_match = both && qcd == acd;
                }
                h = max(dg, max(e, f));
                pay.cell(r, t, i, j, t == 0 || t == B - 1, (dg >= e && dg >= f) ? kFromDiag : (e >= f ? kFromE : kFromF), eo >= ee, fo >= fe, is_match);
                h = max(h, kNeg); e = max(e, kNeg); f = max(f, kNeg);
            } else pay.outside(r, t, i);
            H[r] = h; E[r] = e; F[r] = f;
            pay.joined(r, t, i);
        }
    }
    int best = kNeg, best_t = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int t = lane * R + r;
        if (t < B && H[r] > best) { best = H[r]; best_t = t; }
    }
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const int ob = __shfl_xor(best, sh), ot = __shfl_xor(best_t, sh);
        if (ob > best || (ob == best && ot < best_t)) { best = ob; best_t = ot; }
    }
    if (best < kNoPath) return BandEnd{MP_ANCHOR_NO_SCORE, -1};
    pay.finish(best_t / R, best_t % R);
    return BandEnd{best, best_t};
}

}  // namespace

}  // namespace mp
