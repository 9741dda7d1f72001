// SMO_POISON_LDS (tests; lds_poison.hip): what the knob may hold and the word the fill stores, as plain integer arithmetic.
// Host-only: no HIP type is named here, so g++ alone compiles it and tests/test_lds_poison_cpu.py checks both on the CPU.
#pragma once
#include <cstdint>

namespace smo {
namespace lds {

// SMO_POISON_LDS=<0..255>: digits only (no sign, no blanks, no fraction, no 0x), the rule of SMO_POISON
inline bool parse_byte(const char* s, int* byte) {
    *byte = -1;
    if (!s || !*s) return false;
    int v = 0;
    for (const char* c = s; *c; ++c) {
        if (*c < '0' || *c > '9') return false;
        v = v * 10 + (*c - '0');
        if (v > 255) return false;
    }
    *byte = v;
    return true;
}

// the 8-byte word whose every byte is `byte`: what the fill stores and what the probe compares with
inline uint64_t fill_word(int byte) { return 0x0101010101010101ull * (uint64_t)(byte & 0xFF); }

}  // namespace lds
}  // namespace smo
