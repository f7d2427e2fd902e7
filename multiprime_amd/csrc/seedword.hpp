// seedword.hpp — the letters and 12-mer words of the seeded alignments (anchor.hip, star.hip, cluster.hip): one code per letter, one word
// per position, one hash per word.
#pragma once

#include "common.hpp"
#include "../../include/mprime_anchor.h"

namespace mp {

__host__ __device__ inline int base_code(uint8_t ch) {
    ch &= 0xDF;                                // upper case
    return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
}
__host__ __device__ inline uint32_t word_hash(uint32_t kmer, int log2_slots) { return (kmer * 2654435761u) >> (32 - log2_slots); }

__host__ __device__ inline uint8_t upper_letter(uint8_t ch) { return ch >= 'a' && ch <= 'z' ? (uint8_t)(ch - 32) : ch; }

// the complement of an upper-cased letter: A<>T, C<>G, R<>Y, K<>M, B<>V, D<>H, U->A; S, W, N and every other byte as they are
__host__ __device__ inline uint8_t complement_letter(uint8_t ch) {
    switch (ch) {
        case 'A': return 'T'; case 'T': return 'A'; case 'U': return 'A'; case 'C': return 'G'; case 'G': return 'C';
        case 'R': return 'Y'; case 'Y': return 'R'; case 'K': return 'M'; case 'M': return 'K';
        case 'B': return 'V'; case 'V': return 'B'; case 'D': return 'H'; case 'H': return 'D';
        default: return ch;
    }
}

// The 2-bit word of MP_ANCHOR_WORD letters, the first most significant: code_of(x) is the code of letter x (0 .. 3 for A, C, G, T).
// kEmpty when one of them is not A/C/G/T.
template <class CodeOf>
__host__ __device__ inline uint32_t seed_word(CodeOf code_of) {
    uint32_t w = 0;
    bool ok = true;
#pragma unroll
    for (int x = 0; x < MP_ANCHOR_WORD; x++) {
        const uint32_t cd = (uint32_t)code_of(x);
        ok = ok && cd < 4;
        w = (w << 2) | (cd & 3u);
    }
    return ok ? w : kEmpty;
}
// ... of the codes p[0 .. 12), of the letters p[0 .. 12), and of rc(letters p[0 .. 12)): complemented, in reversed order
__host__ __device__ inline uint32_t seed_word_codes(const uint8_t *p) { return seed_word([p](int x) { return (int)p[x]; }); }
__host__ __device__ inline uint32_t seed_word_letters(const uint8_t *p) { return seed_word([p](int x) { return base_code(p[x]); }); }
__host__ __device__ inline uint32_t seed_word_rc_letters(const uint8_t *p) {
    return seed_word([p](int x) { return base_code(complement_letter(upper_letter(p[MP_ANCHOR_WORD - 1 - x]))); });
}

}  // namespace mp
