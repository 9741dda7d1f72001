// Guard zones around device allocations (SMO_GUARD, tests): the zone-size rule, the pattern and the comparison, as plain integer arithmetic.
// The counterpart of SMO_POISON for WRITES: a kernel that stores one row, slot or member past the block it was handed lands in hipMalloc's
// slack or in the 256-byte rounding of a device vector, where nobody reads it.  With the knob set every block of DevPool::alloc and
// smo_vec_alloc is laid out as
//
//     [front zone Z][block: requested bytes][slack: up to the next multiple of 256][back zone Z][result words of the check]
//
// with Z = clamp(round_up(requested, 256), 4096, cap): as long as the block itself up to the cap, so that a store that is wrong by one whole
// slot, member or component still lands inside it.  Zones and slack hold a position-dependent pattern that is written on the device when the
// block is handed out and compared on the device when it is given back (guard.hip); smo_guard_report adds the results up.
//
// Host-only: no HIP type is named here, so g++ alone compiles it and tests/c/guard_host_test.cpp checks rule, pattern and comparison on the
// CPU (tests/test_guard_host.py).  The two functions the kernels share carry SMO_GUARD_HD, which is a plain `inline` for a host compiler.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SMO_GUARD_HD __host__ __device__ __forceinline__      // (no kernel of the library calls a device function)
#else
#define SMO_GUARD_HD inline
#endif

namespace smo {
namespace guard {

constexpr size_t kAlign = 256;                    // granule of zones and of the rounded block: the pointer handed out keeps hipMalloc's alignment
constexpr size_t kMinZone = 4096;
constexpr size_t kMinCap = 4096, kMaxCap = (size_t)1 << 30;
constexpr size_t kResultBytes = 256;              // behind the back zone: the three words the counting kernel writes

enum Region { FRONT = 1, TAIL = 2 };              // TAIL: slack and back zone, one run of words from the last (partly) requested word on

inline size_t round_up(size_t bytes, size_t to) { return (bytes + to - 1) / to * to; }

// SMO_GUARD=<cap in bytes>: digits only (no sign, no blanks, no fraction), a multiple of 256 in 4096 .. 2^30
inline bool parse_cap(const char* s, size_t* cap) {
    *cap = 0;
    if (!s || !*s) return false;
    size_t v = 0;
    for (const char* c = s; *c; ++c) {
        if (*c < '0' || *c > '9' || c - s >= 11) return false;
        v = v * 10 + (size_t)(*c - '0');
    }
    if (v < kMinCap || v > kMaxCap || v % kAlign != 0) return false;
    *cap = v;
    return true;
}

inline size_t zone_bytes(size_t requested, size_t cap) {
    const size_t z = round_up(requested, kAlign);
    return z < kMinZone ? kMinZone : z > cap ? cap : z;
}
inline size_t slack_bytes(size_t requested) { return round_up(requested, kAlign) - requested; }

// Word i of a region.  The two top bytes differ from each other in every word, so no word is eight equal bytes (zero or any SMO_POISON fill),
// and the 48 bits below them are a bijection of the index (an odd multiplier modulo 2^48), so that a run of guard words copied to another
// place differs from what belongs there and the low bytes are not the zeros of a small index.
SMO_GUARD_HD uint64_t word(int region, uint64_t i) {
    const uint64_t low = (i * 0x9E3779B97F4Bull + 0x6A09E667F3BDull) & 0x0000FFFFFFFFFFFFull;
    return 0xA500000000000000ull | ((uint64_t)(0xC0 | region) << 48) | low;
}
// ... with its first `skip` bytes (the end of the requested bytes inside the first word of TAIL) taken from `keep`
SMO_GUARD_HD uint64_t mask_from(unsigned skip) { return skip == 0 ? ~0ull : skip >= 8 ? 0ull : ~0ull << (8 * skip); }     // little endian
SMO_GUARD_HD uint64_t merged(int region, uint64_t i, unsigned skip, uint64_t keep) {
    const uint64_t m = mask_from(skip);
    return (word(region, i) & m) | (keep & ~m);
}
// first damaged byte of word i (0..7) or 8 when it is intact; the first `skip` bytes are not the guard's
SMO_GUARD_HD unsigned first_bad_byte(int region, uint64_t i, unsigned skip, uint64_t got) {
    const uint64_t diff = (got ^ word(region, i)) & mask_from(skip);
    if (diff == 0) return 8;
    unsigned b = 0;
    while (((diff >> (8 * b)) & 0xFFull) == 0) ++b;
    return b;
}

// Geometry of one guarded block inside its allocation, byte offsets from the allocation's base
struct Layout {
    size_t requested = 0, zone = 0;
    size_t rounded() const { return round_up(requested, kAlign); }
    size_t block() const { return zone; }                                        // the pointer handed out
    size_t tail() const { return zone + (requested & ~(size_t)7); }              // first word of TAIL
    unsigned tail_skip() const { return (unsigned)(requested & 7); }             // requested bytes inside that word
    size_t front_words() const { return zone / 8; }
    size_t tail_words() const { return (zone + rounded() + zone - tail()) / 8; }
    size_t result() const { return zone + rounded() + zone; }
    size_t total() const { return result() + kResultBytes; }
};

struct Damage {
    size_t words = 0;                 // damaged 8-byte words
    size_t first = (size_t)-1;        // byte offset of the first damaged byte from the region's first word; (size_t)-1: none
    bool any() const { return words != 0; }
};

// The comparison on the host (the counting kernel of guard.hip does the same with integer atomics): `words` words of `region` at `got`
inline Damage compare(const unsigned char* got, size_t words, int region, unsigned skip) {
    Damage d;
    for (size_t i = 0; i < words; ++i) {
        uint64_t w = 0;
        for (int b = 7; b >= 0; --b) w = (w << 8) | got[8 * i + b];
        const unsigned bad = first_bad_byte(region, i, i == 0 ? skip : 0, w);
        if (bad < 8) {
            if (!d.any()) d.first = 8 * i + bad;
            ++d.words;
        }
    }
    return d;
}
inline void fill(unsigned char* out, size_t words, int region, unsigned skip) {
    for (size_t i = 0; i < words; ++i) {
        uint64_t keep = 0;
        for (int b = 7; b >= 0; --b) keep = (keep << 8) | out[8 * i + b];
        const uint64_t w = merged(region, i, i == 0 ? skip : 0, keep);
        for (int b = 0; b < 8; ++b) out[8 * i + b] = (unsigned char)(w >> (8 * b));
    }
}

// What a report says about the first damage of a block: the zone's name and the byte offset from the block's start (front zone: negative)
// or from its end, the end of the requested bytes (slack and back zone: 0 is the first byte past the block).
struct Where {
    const char* zone;
    long long offset;
    bool from_start;
};
inline Where where(const Layout& l, const Damage& front, const Damage& tail) {
    if (front.any()) return {"front zone", (long long)front.first - (long long)l.zone, true};
    const size_t past = tail.first - l.tail_skip();                              // bytes past the end of the requested bytes
    return {past < slack_bytes(l.requested) ? "slack" : "back zone", (long long)past, false};
}

}  // namespace guard
}  // namespace smo
