// Host check of the guard zones of SMO_GUARD (spheremanopt_amd/csrc/guard.hpp), run by tests/test_guard_host.py as a program of its own: the
// zone-size rule at its three regimes and their boundaries, the knob's values, the pattern (no word equals zero or a poison fill, no two
// positions hold the same word), and the comparison on a host copy of a block's layout: one damaged byte at the first, the last and an
// interior position of each zone is found at that offset, damage in slack of every length is found, an intact block reports nothing.  One
// line "ok <group>" per group, "FAIL ..." on any violation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "guard.hpp"

using namespace smo::guard;

static int fails = 0;
#define REQUIRE(cond, ...)                                       \
    do {                                                         \
        if (!(cond)) {                                           \
            if (fails < 20) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } \
            ++fails;                                             \
        }                                                        \
    } while (0)

static void group(const char* name, int before, long cases) { if (fails == before) std::printf("ok %s (%ld cases)\n", name, cases); }

// a host copy of one guarded allocation: the block holds `fill`, zones and slack the pattern
struct HostBlock {
    Layout l;
    std::vector<unsigned char> mem;
    HostBlock(size_t requested, size_t cap, unsigned char fill_byte) {
        l.requested = requested; l.zone = zone_bytes(requested, cap);
        mem.assign(l.total(), fill_byte);
        fill(mem.data(), l.front_words(), FRONT, 0);
        fill(mem.data() + l.tail(), l.tail_words(), TAIL, l.tail_skip());
    }
    Damage front() const { return compare(mem.data(), l.front_words(), FRONT, 0); }
    Damage tail() const { return compare(mem.data() + l.tail(), l.tail_words(), TAIL, l.tail_skip()); }
    unsigned char* block() { return mem.data() + l.block(); }
};

int main() {
    const size_t cap = 64 * 1024;
    long cases = 0;

    // ---- the knob ---------------------------------------------------------------------------------------------------------------------------
    int before = fails;
    {
        size_t v = 0;
        for (const char* bad : {"100", "0", "-4096", "4096.0", "", " 4096", "2147483648", "4097", "4096 ", "0x1000", "+4096", "99999999999999999999999"}) {
            REQUIRE(!parse_cap(bad, &v) && v == 0, "parse_cap accepts \"%s\" (%zu)", bad, v); ++cases;
        }
        REQUIRE(!parse_cap(nullptr, &v), "parse_cap accepts null"); ++cases;
        for (const char* good : {"4096", "4352", "67108864", "1073741824"}) {
            REQUIRE(parse_cap(good, &v) && v == (size_t)std::strtoull(good, nullptr, 10), "parse_cap refuses \"%s\"", good); ++cases;
        }
        REQUIRE(!parse_cap("1073742080", &v), "parse_cap accepts 2^30 + 256"); ++cases;
    }
    group("knob", before, cases);

    // ---- the zone rule: clamp(round_up(requested, 256), 4096, cap) -------------------------------------------------------------------------------
    before = fails; cases = 0;
    {
        struct { size_t req, zone; } want[] = {{1, 4096}, {255, 4096}, {256, 4096}, {257, 4096}, {4095, 4096}, {4096, 4096}, {4097, 4352},
                                                {8192, 8192}, {cap - 256, cap - 256}, {cap - 255, cap}, {cap - 1, cap}, {cap, cap}, {cap + 1, cap},
                                                {100 * cap, cap}};
        for (auto& w : want) {
            REQUIRE(zone_bytes(w.req, cap) == w.zone, "zone_bytes(%zu, %zu) = %zu, expected %zu", w.req, cap, zone_bytes(w.req, cap), w.zone); ++cases;
        }
        REQUIRE(zone_bytes(1, 4096) == 4096 && zone_bytes(1 << 20, 4096) == 4096, "a cap of 4096 leaves one zone size"); ++cases;
        for (size_t req = 1; req <= 3 * cap; req += 37) {
            const size_t z = zone_bytes(req, cap);
            Layout l; l.requested = req; l.zone = z;
            REQUIRE(z % kAlign == 0 && z >= kMinZone && z <= cap && (z >= req || z == cap), "zone %zu of %zu requested bytes", z, req);
            REQUIRE(l.block() % kAlign == 0 && l.rounded() - req == slack_bytes(req) && slack_bytes(req) < kAlign, "layout of %zu bytes", req);
            REQUIRE(l.tail() % 8 == 0 && l.tail() + l.tail_skip() == l.block() + req && 8 * l.tail_words() + l.tail() == l.result() &&
                    l.result() % kAlign == 0 && l.total() == 2 * z + l.rounded() + kResultBytes, "tail of %zu bytes", req);
            ++cases;
        }
    }
    group("zone rule", before, cases);

    // ---- the pattern ------------------------------------------------------------------------------------------------------------------------------
    before = fails; cases = 0;
    {
        std::set<uint64_t> seen;
        for (int region : {FRONT, TAIL})
            for (uint64_t i = 0; i < (1u << 17); ++i) {
                const uint64_t w = word(region, i);
                bool uniform = true;
                for (int b = 1; b < 8; ++b) uniform = uniform && ((w >> (8 * b)) & 0xFF) == (w & 0xFF);
                REQUIRE(!uniform, "word %llu of region %d is eight equal bytes", (unsigned long long)i, region);      // zero and EVERY poison fill
                for (uint64_t fillb : {0x00ull, 0xFFull, 0x3Full}) REQUIRE(w != fillb * 0x0101010101010101ull, "word %llu equals a fill", (unsigned long long)i);
                REQUIRE(seen.insert(w).second, "word %llu of region %d repeats", (unsigned long long)i, region);
                ++cases;
            }
        // the largest indices of a 2^30 zone keep the property
        for (uint64_t i : {(uint64_t)(kMaxCap / 8 - 1), (uint64_t)(2 * kMaxCap / 8 + 31)}) {
            const uint64_t w = word(TAIL, i);
            REQUIRE((w >> 56) == 0xA5 && ((w >> 48) & 0xFF) == 0xC2 && w != word(TAIL, i - 1) && w != word(FRONT, i), "word %llu", (unsigned long long)i); ++cases;
        }
        // a run of guard words copied elsewhere does not match
        HostBlock hb(1024, cap, 0x11);
        std::memcpy(hb.mem.data() + 64, hb.mem.data(), 64);
        REQUIRE(hb.front().words == 8 && hb.front().first / 8 == 8, "a copied run: %zu words from %zu", hb.front().words, hb.front().first); ++cases;
    }
    group("pattern", before, cases);

    // ---- intact blocks: nothing reported, whatever the block holds -----------------------------------------------------------------------------------------
    before = fails; cases = 0;
    for (size_t req : {(size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)264, (size_t)4096, cap - 1, cap, cap + 1})
        for (unsigned char fb : {0x00, 0xFF, 0x3F, 0xA5}) {
            HostBlock hb(req, cap, fb);
            REQUIRE(!hb.front().any() && !hb.tail().any() && hb.front().first == (size_t)-1, "intact block of %zu bytes reports damage", req);
            std::memset(hb.block(), fb ^ 0x5A, req);                  // writing every requested byte damages nothing
            REQUIRE(!hb.front().any() && !hb.tail().any(), "writing the %zu requested bytes damages a zone", req);
            ++cases;
        }
    group("intact", before, cases);

    // ---- one damaged byte at the first, the last and an interior position of each zone ----------------------------------------------------------------------
    before = fails; cases = 0;
    for (size_t req : {(size_t)1, (size_t)264, (size_t)4096, (size_t)5003, cap + 1}) {
        const Layout l = HostBlock(req, cap, 0).l;
        const size_t slack = slack_bytes(req);
        for (size_t pos : {(size_t)0, l.zone / 2 + 3, l.zone - 1}) {
            HostBlock f(req, cap, 0x3F);                             // front zone, byte `pos` of it
            f.mem[pos] ^= 0x80;
            const Damage d = f.front();
            const Where w = where(f.l, d, f.tail());
            REQUIRE(d.words == 1 && d.first == pos && !f.tail().any(), "front byte %zu of a %zu-byte block: %zu words, first %zu", pos, req, d.words, d.first);
            REQUIRE(std::strcmp(w.zone, "front zone") == 0 && w.from_start && w.offset == (long long)pos - (long long)l.zone, "front byte %zu named %s%+lld", pos, w.zone, w.offset);
            HostBlock b(req, cap, 0x3F);                             // back zone, byte `pos` of it
            b.mem[l.block() + l.rounded() + pos] ^= 0x01;
            const Damage t = b.tail();
            const Where v = where(b.l, b.front(), t);
            REQUIRE(t.words == 1 && !b.front().any() && std::strcmp(v.zone, "back zone") == 0 && !v.from_start && v.offset == (long long)(slack + pos),
                    "back byte %zu of a %zu-byte block: %zu words, %s%+lld", pos, req, t.words, v.zone, v.offset);
            cases += 2;
        }
    }
    group("single byte", before, cases);

    // ---- slack of every length 0 .. 248 (and the lengths between, which a DevPool block of bytes or ints has) --------------------------------------------------
    before = fails; cases = 0;
    for (size_t slack = 0; slack < 256; ++slack) {
        const size_t req = 2048 - slack;
        REQUIRE(slack_bytes(req) == slack, "slack_bytes(%zu)", req);
        for (size_t pos : {(size_t)0, slack / 2, slack ? slack - 1 : 0}) {
            HostBlock hb(req, cap, 0xFF);
            if (slack == 0) {                                        // no slack: the first byte past the block is the back zone's first
                hb.mem[hb.l.block() + req] ^= 0x10;
                const Where w = where(hb.l, hb.front(), hb.tail());
                REQUIRE(hb.tail().words == 1 && std::strcmp(w.zone, "back zone") == 0 && w.offset == 0, "no slack: %s%+lld", w.zone, w.offset);
            } else {
                hb.mem[hb.l.block() + req + pos] ^= 0x10;
                const Where w = where(hb.l, hb.front(), hb.tail());
                REQUIRE(hb.tail().words == 1 && std::strcmp(w.zone, "slack") == 0 && w.offset == (long long)pos, "slack %zu byte %zu: %zu words, %s%+lld", slack, pos,
                        hb.tail().words, w.zone, w.offset);
                hb.mem[hb.l.block() + req - 1] ^= 0x10;              // the last requested byte, in the same word when req % 8 != 0: not the guard's
                REQUIRE(hb.tail().words == 1, "slack %zu: the last requested byte counts as damage", slack);
            }
            ++cases;
        }
        // every slack byte at once, and one word of the back zone: counted in words
        HostBlock hb(req, cap, 0x00);
        std::memset(hb.mem.data() + hb.l.block() + req, 0, slack + 8);
        REQUIRE(hb.tail().words == (hb.l.block() + hb.l.rounded() + 8 - hb.l.tail()) / 8, "slack %zu zeroed: %zu words", slack, hb.tail().words);
        REQUIRE(hb.tail().first >= hb.l.tail_skip() && hb.tail().first < 8, "slack %zu zeroed: first %zu", slack, hb.tail().first);      // (byte 7 is 0xA5)
        ++cases;
    }
    group("slack", before, cases);

    std::printf(fails ? "FAILED (%d)\n" : "all ok\n", fails);
    return fails ? 1 : 0;
}
