// seedword.hpp — the letters and 12-mer words of the seeded alignments (anchor.hip, cluster.hip): one code per letter, one hash per word.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace mp {

__host__ __device__ inline int base_code(uint8_t ch) {
    ch &= 0xDF;                                // upper case
    return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
}
__host__ __device__ inline uint32_t word_hash(uint32_t kmer, int log2_slots) { return (kmer * 2654435761u) >> (32 - log2_slots); }

}  // namespace mp
