// ont_emul.cpp — the device's pair routine (multiprime_amd/csrc/ontcore.hpp) on the CPU: reads lines "a<TAB>b" (either side may be
// empty; any byte other than A, C, G, T stands for "no base") and prints M(a, b) per line, from 64-bit masks and — where both sides have at most 32 bytes — from 32-bit masks too (they must agree).  tests/test_ont.py builds it with g++ and
// compares with difflib, so the bit-mask walk is checked where there is no GPU.
//   g++ -O2 -std=c++17 -o ont_emul tools/ont_emul.cpp
#include <cstdio>
#include <iostream>
#include <string>

#include "../multiprime_amd/csrc/ontcore.hpp"

int main() {
    std::string line;
    uint32_t stack[MP_ONT_STACK], stack32[MP_ONT_STACK / 2 + 1];    // (a sanitizer build sees a push past either)
    while (std::getline(std::cin, line)) {
        const size_t tab = line.find('\t');
        if (tab == std::string::npos) { fprintf(stderr, "ont_emul: a line without a tab\n"); return 2; }
        const std::string a = line.substr(0, tab), b = line.substr(tab + 1);
        if (a.size() > MP_ONT_MAX_LEN || b.size() > MP_ONT_MAX_LEN) { fprintf(stderr, "ont_emul: more than %d bytes\n", MP_ONT_MAX_LEN); return 2; }
        uint64_t pa[4], kb[4];
        mp::ont_masks((const uint8_t *)a.data(), (int)a.size(), pa);
        mp::ont_masks((const uint8_t *)b.data(), (int)b.size(), kb);
        const int m = mp::ont_matches<uint64_t>(pa, (int)a.size(), kb, (int)b.size(), stack, 1);
        if (a.size() <= 32 && b.size() <= 32) {          // the 32-bit form of the same routine must agree
            const uint32_t pa32[4] = {(uint32_t)pa[0], (uint32_t)pa[1], (uint32_t)pa[2], (uint32_t)pa[3]};
            const uint32_t kb32[4] = {(uint32_t)kb[0], (uint32_t)kb[1], (uint32_t)kb[2], (uint32_t)kb[3]};
            const int m32 = mp::ont_matches<uint32_t>(pa32, (int)a.size(), kb32, (int)b.size(), stack32, 1);
            if (m32 != m) { fprintf(stderr, "ont_emul: %s / %s: %d with 64-bit masks, %d with 32-bit masks\n", a.c_str(), b.c_str(), m, m32); return 3; }
        }
        printf("%d\n", m);
    }
    return 0;
}
