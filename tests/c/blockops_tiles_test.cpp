// Host check of the chunk / tile index arithmetic the block kernels use (spheremanopt_amd/csrc/blockops_tiles.hpp), run by
// tests/test_blockops_cpu.py as a program of its own.  For every (B, n) it walks block_gram's loader exactly as the kernel does — workgroup,
// chunk iteration, pass, lane, half of the pair — and requires that every (member, element) pair is owned exactly once, that the inverse map
// gram_owner names that owner, that everything else the walk visits is flagged as padding, and that every MFMA operand lane at or beyond the
// block's member count is flagged.  The same for block_combine's element ownership.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blockops_tiles.hpp"

using namespace smo::blockops;

static int fails = 0;
#define REQUIRE(cond, ...)                                       \
    do {                                                         \
        if (!(cond)) {                                           \
            if (fails < 20) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } \
            ++fails;                                             \
        }                                                        \
    } while (0)

static void check(int B, size_t n) {
    const GramPlan p = gram_plan(B, n);
    REQUIRE(p.nt >= 1 && p.nt <= 4 && p.kc == chunk_len(B < kBlock ? B : kBlock) && p.kc % (kKStep * kWaves) == 0, "plan B=%d n=%zu: nt=%d kc=%d", B, n, p.nt, p.kc);
    REQUIRE(p.nwg >= 1 && p.nwg <= 1024 && (size_t)p.nwg * p.cpw >= p.nchunks && (size_t)(p.nwg - 1) * p.cpw < p.nchunks, "plan B=%d n=%zu: nwg=%d cpw=%zu nchunks=%zu",
            B, n, p.nwg, p.cpw, p.nchunks);
    REQUIRE(p.nblk * kBlock >= B && (p.nblk - 1) * kBlock < B, "plan B=%d: nblk=%d", B, p.nblk);
    const int image = 2 * lds_rows(p.kc) * lds_stride(p.kc);                // doubles of LDS: both operands
    REQUIRE(lds_stride(p.kc) % 2 == 0 && kTile * p.nt * kTile * p.nt <= image && image * 8 <= 65536, "LDS image nt=%d kc=%d", p.nt, p.kc);
    int members = 0;
    for (int blk = 0; blk < p.nblk; ++blk) {
        const int rows = block_rows(p, blk);
        REQUIRE(rows >= 1 && rows <= kTile * p.nt && rows < lds_rows(p.kc), "B=%d block %d: %d rows for %d tiles, %d image rows", B, blk, rows, p.nt, lds_rows(p.kc));
        REQUIRE(gram_passes(p, rows) <= max_passes(p.kc), "B=%d block %d: %d passes > %d", B, blk, gram_passes(p, rows), max_passes(p.kc));
        members += rows;
        std::vector<int> owned((size_t)rows * n, 0);
        for (int wg = 0; wg < p.nwg; ++wg)
            for (size_t iter = 0; iter < p.cpw; ++iter) {
                const size_t chunk = (size_t)wg * p.cpw + iter;
                if (chunk >= p.nchunks) break;
                for (int pass = 0; pass < max_passes(p.kc); ++pass)
                    for (int lane = 0; lane < kThreads; ++lane) {
                        const GramItem it = gram_item(p, chunk, pass, lane);
                        REQUIRE(it.col >= 0 && it.col + 1 < p.kc && it.col % 2 == 0, "item col %d", it.col);
                        for (int half = 0; half < 2; ++half) {
                            const size_t k = it.k + half;
                            const bool pad = row_is_padding(it.row, rows) || elem_is_padding(k, n);
                            if (it.row < rows && k < n) {
                                REQUIRE(!pad, "B=%d n=%zu: member %d element %zu flagged as padding", B, n, it.row, k);
                                owned[(size_t)it.row * n + k] += 1;
                                const GramOwner o = gram_owner(p, it.row, k);
                                REQUIRE(o.wg == wg && o.iter == iter && o.pass == pass && o.lane == lane && o.half == half,
                                        "B=%d n=%zu: owner of (%d, %zu) is (%d,%zu,%d,%d,%d), the walk met it at (%d,%zu,%d,%d,%d)", B, n, it.row, k, o.wg, o.iter,
                                        o.pass, o.lane, o.half, wg, iter, pass, lane, half);
                            } else {
                                REQUIRE(pad, "B=%d n=%zu: row %d element %zu is outside the data and not flagged", B, n, it.row, k);
                            }
                        }
                    }
            }
        for (size_t i = 0; i < owned.size(); ++i) REQUIRE(owned[i] == 1, "B=%d n=%zu block %d: member %zu element %zu owned %d times", B, n, blk, i / n, i % n, owned[i]);
        // MFMA operand lanes: rows at or beyond the member count are padding and read the zero row of the LDS image
        for (int t = 0; t < p.nt; ++t)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = mfma_row(t, lane);
                REQUIRE(r >= 0 && r < kTile * p.nt, "mfma row %d", r);
                REQUIRE(row_is_padding(r, rows) == (r >= rows), "B=%d block %d: operand row %d padding flag", B, blk, r);
                // a padded operand row reads the zero row behind the members, which no loader item writes; a member row reads itself
                REQUIRE(lds_row(r, rows, p.kc) == (r >= rows ? lds_rows(p.kc) - 1 : r) && lds_rows(p.kc) - 1 >= rows, "B=%d block %d: row %d lives in %d", B, blk, r,
                        lds_row(r, rows, p.kc));
                for (int s = 0; s < p.kc / kKStep; ++s) REQUIRE(mfma_col(s, lane) >= 0 && mfma_col(s, lane) < p.kc, "mfma col");
            }
    }
    REQUIRE(members == B, "B=%d: the blocks hold %d members", B, members);
    // accumulator map: the 64 lanes x 4 registers are the 256 entries of a tile, once each
    std::vector<int> seen(kTile * kTile, 0);
    for (int lane = 0; lane < 64; ++lane)
        for (int v = 0; v < 4; ++v) seen[acc_row(lane, v) * kTile + acc_col(lane)] += 1;
    for (int i = 0; i < kTile * kTile; ++i) REQUIRE(seen[i] == 1, "accumulator entry %d held %d times", i, seen[i]);
    // block_combine: element ownership and the register tile
    std::vector<int> el(n, 0);
    for (size_t wg = 0; wg < combine_wgs(n); ++wg)
        for (int lane = 0; lane < kThreads; ++lane) {
            const size_t k = combine_elem(wg, lane);
            if (!elem_is_padding(k, n)) el[k] += 1;
            else REQUIRE(k >= n, "combine padding");
        }
    for (size_t k = 0; k < n; ++k) REQUIRE(el[k] == 1, "combine: element %zu owned %d times", k, el[k]);
    const int nb = combine_cols(B);
    REQUIRE(nb <= kCombineCols && (B > kCombineCols ? nb == kCombineCols : nb >= B), "combine_cols(%d) = %d", B, nb);
}

int main() {
    const int Bs[] = {1, 2, 3, 16, 17, 33, 64, 65};
    std::vector<size_t> ns;
    for (size_t n = 1; n <= 70; ++n) ns.push_back(n);
    ns.push_back(2187); ns.push_back(5184); ns.push_back(10125);
    int cases = 0;
    for (int B : Bs)
        for (size_t n : ns) { check(B, n); ++cases; }
    for (int B : {3, 17, 256}) { check(B, 139968); ++cases; }      // G = 36: more than one chunk per workgroup, the largest batch
    std::printf("%s %d cases, %d failures\n", fails ? "FAIL" : "ok", cases, fails);
    return fails ? 1 : 0;
}
