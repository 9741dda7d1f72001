// Chunk and tile index arithmetic of the cross-member block kernels (blockops.hip: block_gram, block_combine).
//
// Host-compilable: the kernels and tests/c/blockops_tiles_test.cpp include this one file, so "which workgroup, iteration and lane owns
// element k of member a, and which lanes are padding" has a single answer.
//
// block_gram works on a 64 x 64 block of members (row block = members of x, column block = members of y).  A workgroup of 256 lanes owns a
// CONTIGUOUS range of element chunks; per chunk it stages, for every valid member of the block, `chunk_len` elements in LDS as
// [member row][chunk_len + kLdsPad] (chunk_len by member count) and its four waves split the chunk's k steps of v_mfma_f64_16x16x4_f64 among themselves (wave w takes the
// steps s = w, w + 4, ...), each over all tiles.  A loader ITEM is one (member row, element pair); item i of a chunk belongs to lane i % 256
// in pass i / 256.  Rows at or beyond the block's member count and elements at or beyond n are PADDING: never read from memory, zero in LDS.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define SMO_BO_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SMO_BO_HD inline
#endif

namespace smo {
namespace blockops {

constexpr int kThreads = 256;      // lanes per workgroup (4 waves)
constexpr int kWaves = 4;
constexpr int kBlock = 64;         // members per block side
constexpr int kTile = 16;          // MFMA tile side
constexpr int kKStep = 4;          // k extent of one v_mfma_f64_16x16x4_f64
constexpr int kLdsPad = 4;         // row stride = chunk_len + 4 doubles: 16-byte aligned rows, and the 16 rows x 4 k of one MFMA operand read
                                   // fall on the 32 eight-byte bank pairs exactly twice (the minimum for 64 lanes)
constexpr int kMaxBatch = 256;     // members a context may have for these operations
constexpr int kCombineCols = 64;   // output members per workgroup column block of block_combine

// 16-row tiles per block side for `members` (<= kBlock) members: 1..4
SMO_BO_HD constexpr int tiles_for(int members) { return (members + kTile - 1) / kTile; }
// elements per chunk for a block of `members` (<= kBlock) members: members x chunk_len stays near 2048 elements, i.e. 16 KB per operand and
// workgroup in flight whatever the member count (a few members with short chunks leave the loads latency-bound)
SMO_BO_HD constexpr int chunk_len(int members) { return members <= 4 ? 512 : members <= 8 ? 256 : members <= 16 ? 128 : members <= 32 ? 64 : 32; }
SMO_BO_HD constexpr int lds_stride(int kc) { return kc + kLdsPad; }
// rows of the LDS image [row][chunk_len + pad] of one operand: the most members that take this chunk length, and ONE zero row behind them that
// every padded MFMA operand row reads (lds_row)
SMO_BO_HD constexpr int lds_rows(int kc) { return (kc >= 512 ? 4 : kc >= 256 ? 8 : kc >= 128 ? 16 : kc >= 64 ? 32 : kBlock) + 1; }
// loader passes that cover the image: 4 for every chunk length
SMO_BO_HD constexpr int max_passes(int kc) { return ((lds_rows(kc) - 1) * (kc / 2) + kThreads - 1) / kThreads; }

struct GramPlan {
    int B;                 // members
    int nt;                // tiles per block side
    int kc;                // chunk_len(min(B, 64))
    int nblk;              // 64-member blocks per side
    int nwg;               // workgroups along the element axis (= partial blocks per entry)
    size_t n;              // elements per member (= member stride)
    size_t nchunks;        // ceil(n / kc)
    size_t cpw;            // chunks per workgroup: workgroup g owns chunks [g cpw, (g + 1) cpw)
};

SMO_BO_HD GramPlan gram_plan(int B, size_t n) {
    GramPlan p;
    p.B = B;
    p.n = n;
    p.nt = tiles_for(B < kBlock ? B : kBlock);
    p.kc = chunk_len(B < kBlock ? B : kBlock);
    p.nblk = (B + kBlock - 1) / kBlock;
    p.nchunks = (n + (size_t)p.kc - 1) / (size_t)p.kc;
    // the partial blocks [nwg][B][B] are written and read once more: keep them near 16 MB (2^21 doubles), between 64 and 1024 workgroups
    size_t cap = ((size_t)1 << 21) / ((size_t)B * (size_t)B);
    cap = cap < 64 ? 64 : cap > 1024 ? 1024 : cap;
    size_t nwg = p.nchunks < cap ? p.nchunks : cap;
    if (nwg < 1) nwg = 1;
    p.cpw = (p.nchunks + nwg - 1) / nwg;
    if (p.cpw < 1) p.cpw = 1;
    p.nwg = (int)((p.nchunks + p.cpw - 1) / p.cpw);
    if (p.nwg < 1) p.nwg = 1;
    return p;
}

// members of block `blk` (0 .. nblk - 1)
SMO_BO_HD int block_rows(const GramPlan& p, int blk) { const int r = p.B - blk * kBlock; return r < kBlock ? r : kBlock; }
// loader passes a block of `rows` members needs per chunk
SMO_BO_HD int gram_passes(const GramPlan& p, int rows) { return (rows * (p.kc / 2) + kThreads - 1) / kThreads; }

struct GramItem {
    int row;               // member row inside the block
    int col;               // first element of the pair inside the chunk (even)
    size_t k;              // ... and inside the member
};
// the item of lane `lane` in pass `pass` of chunk `chunk`
SMO_BO_HD GramItem gram_item(const GramPlan& p, size_t chunk, int pass, int lane) {
    const int hp = p.kc / 2, i = pass * kThreads + lane;
    GramItem it;
    it.row = i / hp;
    it.col = 2 * (i % hp);
    it.k = chunk * (size_t)p.kc + (size_t)it.col;
    return it;
}
SMO_BO_HD bool row_is_padding(int row, int rows) { return row >= rows; }
SMO_BO_HD bool elem_is_padding(size_t k, size_t n) { return k >= n; }

struct GramOwner { int wg; size_t iter; int pass, lane, half; };
// who loads element k of member row `row` of a block
SMO_BO_HD GramOwner gram_owner(const GramPlan& p, int row, size_t k) {
    const size_t chunk = k / (size_t)p.kc;
    const int col = (int)(k % (size_t)p.kc), i = row * (p.kc / 2) + col / 2;
    GramOwner o;
    o.wg = (int)(chunk / p.cpw);
    o.iter = chunk % p.cpw;
    o.pass = i / kThreads;
    o.lane = i % kThreads;
    o.half = col & 1;
    return o;
}

// MFMA operand of lane `lane` (0..63) for tile `t`, k step `s` of a chunk: member row and column; lds_row: where that row lives in the image
SMO_BO_HD int mfma_row(int t, int lane) { return kTile * t + (lane & 15); }
SMO_BO_HD int mfma_col(int s, int lane) { return kKStep * s + (lane >> 4); }
SMO_BO_HD int lds_row(int row, int rows, int kc) { return row_is_padding(row, rows) ? lds_rows(kc) - 1 : row; }
// accumulator register v (0..3) of lane `lane`: row and column inside the 16 x 16 tile
SMO_BO_HD int acc_row(int lane, int v) { return (lane >> 4) + 4 * v; }
SMO_BO_HD int acc_col(int lane) { return lane & 15; }

// block_combine: lane t of workgroup g owns element g * 256 + t of every output member of its column block
SMO_BO_HD size_t combine_elem(size_t wg, int lane) { return wg * (size_t)kThreads + (size_t)lane; }
SMO_BO_HD size_t combine_wgs(size_t n) { return (n + kThreads - 1) / kThreads; }
// output columns a workgroup computes (compile-time register tile): the smallest of 4, 16, 32, 64 that holds min(B, 64)
SMO_BO_HD int combine_cols(int B) { return B <= 4 ? 4 : B <= 16 ? 16 : B <= 32 ? 32 : kCombineCols; }

}  // namespace blockops
}  // namespace smo
