// KDYN — 3-D triply-periodic kinematic dynamo: CNAB1 forward solve of the induction equation and the discrete /
// continuous adjoint sweep giving dJ/dB0 and dJ/dU.
//
// Replaces FWD_Solve_IVP_Lin / Compatib_Cond / ADJ_Solve_IVP_Lin / Inner_Prod_3 of
// Example_Problems/Periodic_Domain(Fourier)/Kinematic_Dynamo/FWD_Solve_KDyn.py (:529-689, :696-764, :766-1004,
// :173-181); recurrences: SURVEY.md Appendix A.2.
//
// Data layout in HBM (N = npts, a = N/2 kx modes, m = N-1 ky/kz modes, G = 3N/2 grid points per axis):
//   coefficient fields  C [3][a][m][m]   complex128, kz fastest      (snapshot stack: [n][3][a][m][m])
//   after the z pass    Tz[3][a][m][G]   complex128, z fastest       (slab exchange layout: [peer][field group][3][a/W][m][G/W])
//   after the y pass    Ty[3][a][G*G+8]  complex128, z fastest       (slabs: [3][a][G*G/W+8], all kx, local z planes; the 8 elements of
//                                                                     padding keep a tile's 3a runs off one HBM channel)
//   grid fields         U [3][G][G][G]   float64,    z fastest       (= the reference's flat X vectors; slabs: [3][G][G][G/W])
// Slab decomposition (W ranks): coefficient space is split over kx, grid space over z.  The z passes run on the kx slab, the y
// and x passes on the z slab, and the exchange sits between the z and the y pass, where the data is smallest (16*a*m*G bytes per
// component instead of 16*a*G*G after the y pass).  With W = 1 the "exchange buffer" is simply Tz.
// One 3-D transform = three 1-D passes (z contiguous, y strided, x strided).  Every pass reads HBM in its first
// Stockham stage (zero padding folded into the load) and writes HBM in its last (truncation folded into the store).
// Fusions per time step (4 kernels per forward step, 4 per adjoint step):
//   x pass  : c2r (two real lines per complex FFT) -> cross product with U (and B_f) on the grid -> r2c, one kernel; the last
//             inverse stage, the products and the first forward stage run in registers
//   z pass  : forward z transform -> i k x (.) -> Leray projection -> CNAB1 update -> next state written straight
//             into the snapshot stack (the stack IS the state; no copy) -> inverse z transform of that state (adjoint: of its
//             curl) for the next step, on the same tile
//   nu      : the adjoint's second product is summed over the steps on the grid side (x-transformed) and transformed once
#include <algorithm>
#include <chrono>
#include <type_traits>

#include "comm.hpp"
#include "fft_lds.hpp"
#include "kdyn_plan.hpp"

namespace smo {
namespace {

// ---------------------------------------------------------------------------------------------------------
// Tuning knobs: every compile-time choice of the kernels below that is still a live one, each defined here and nowhere else.  All can be
// overridden with -D (tools/kernel_resources.sh, tools/build_variant.sh are the tuning loop); a value may be an expression in L, the
// transform length G = 3N/2, because the knobs are read in one place only: Shape<L> below, whose members the kernels and the launches use.
// (Variants that were measured and rejected are not switches any more: HISTORY.md lists them and where their measurements are.)
// ---------------------------------------------------------------------------------------------------------
constexpr bool only_2_and_3(int n) { while (n % 2 == 0) n /= 2; while (n % 3 == 0) n /= 3; return n == 1; }

// z passes: ONE row triple per workgroup (3 FFTs).  G <= 192: 192 threads — every butterfly stage of 192 = 4*4*4*3 is then exactly one round
// (144 radix-4 / 192 radix-3 butterflies; with two row triples on 256 threads every stage took two rounds, the second 12-50 % full):
// update kernels 49.7-50.2 / 49.0-49.3 -> 48.7 / 47.0-47.5 us at 128^3.  G > 192: 256 threads (192 / 320 / 384 are 5-8 % slower there).
#ifndef SMO_Z_NBT
#define SMO_Z_NBT 1
#endif
#ifndef SMO_Z_THREADS
#define SMO_Z_THREADS (L > 192 ? 256 : 192)
#endif
// z passes: half twiddle table (the other half is its negative) from this length on: 24.6 -> 21.5 KB at G = 384, seven workgroups per CU instead
// of six (256^3: z_inverse<curl> 256.8 -> 223.4 us, fwd_update 426.2 -> 418.3, adj_update unchanged)
#ifndef SMO_Z_HALF_TW_MIN_L
#define SMO_Z_HALF_TW_MIN_L 200
#endif
// y pass: z columns per workgroup = one 128-byte line; 25 KB (G = 192) / 49 KB (G = 384) of LDS => 5 / 3 workgroups per CU
#ifndef SMO_Y_ZT
#define SMO_Y_ZT 8
#endif
// y pass: half twiddle table from this length on: at G = 384 the 8-column tile + the full table is 55.3 KB — two workgroups per CU, 2.96 would
// fit —, with half a table 52.2 KB: three.  Round 4, 256^3, same box: y<inv> 310.0 -> 299.4 us, y<fwd> 285.5 -> 270.9; at G = 192 (five -> six
// workgroups per CU) nothing moves, so the full table stays there (and the results of the smaller grids as they were)
#ifndef SMO_Y_HALF_TW_MIN_L
#define SMO_Y_HALF_TW_MIN_L 200
#endif
// x passes: waves per SIMD the kernels are built for (amdgpu_waves_per_eu); the sequential adjoint pass has a figure of its own
#ifndef SMO_X_WAVES
#define SMO_X_WAVES 3
#endif
#ifndef SMO_X_SEQ_WAVES
#define SMO_X_SEQ_WAVES SMO_X_WAVES
#endif
// forward x pass, threads: 256 = one middle-section item per thread (HP * G/3 = 256), 102-105 VGPRs => 4 waves per SIMD = 16 per CU
// (192 threads: 148-154 VGPRs, 12 per CU): -5..-7 % on this kernel
#ifndef SMO_X_FWD_NT
#define SMO_X_FWD_NT 256
#endif
// forward x pass, radix policy: butterflies up to radix 8 (192 = 8*8*3, 384 = 8*8*2*3: one LDS round trip and one barrier less per direction;
// 117-120 VGPRs, still four waves per SIMD): -3 % at G = 192, -5 % at G = 384.  The adjoint passes (no registers to spare) and the z / y passes
// get slower with it and keep radix 4.
#ifndef SMO_X_FWD_RADIX
#define SMO_X_FWD_RADIX 8
#endif
// adjoint x pass with both field groups in the tile (X_FUSED_ADJ), threads
#ifndef SMO_X_ADJ_NT
#define SMO_X_ADJ_NT 192
#endif
// sequential adjoint x pass, threads (experiments: 320, 384; profiles/r03_adj_seq_thread_sweep.txt); Shape<L>::XSNT raises it to one thread per item
#ifndef SMO_X_SEQ_NT
#define SMO_X_SEQ_NT SMO_X_FWD_NT
#endif
// sequential adjoint x pass, middle-section items (j, line pair) per thread — the shape of its workgroup:
//   1: one item per thread (256 threads = four waves at G = 192), built for SMO_X_SEQ_WAVES waves per SIMD => three tiles per CU;
//   2: TWO items per thread on 128 threads = two waves, built for two waves per SIMD (up to 256 VGPRs) => FOUR 40-KB tiles per CU, as the
//      forward pass has; every barrier joins two waves, every thread carries two independent butterfly / request chains.  Same tile, same
//      arithmetic per element, same bits.  Only where a tile has 256 items (G = 192; G = 384 with its half tiles); a length that takes it
//      keeps the one-item kernel beside it (KDynEnv::seq_items: the tests compare the two).
//      G = 192: 256 VGPRs, no spills, every early request kept, -5 % on the kernel, -1.5 % per gradient at 128^3; G = 384: 43 registers
//      spilled, not enabled (profiles/r15_kdyn_adj_x_two_wave_resources.txt).
// -DSMO_X_SEQ_ITEMS=1 / =2 forces one shape at every length that can take it (A/B builds from one tree).
#ifndef SMO_X_SEQ_ITEMS
#define SMO_X_SEQ_ITEMS (L == 192 ? 2 : 1)
#endif
// Radix policy of the adjoint x passes (both forms: the same arithmetic per element, bit-identical results): butterflies up to radix 8 where the
// registers of the sequential form allow it — in the inverse heads at G <= 192 (165 VGPRs, -2.3 %), in the forward tails at G = 288, 384 (168,
// -1.5 %); the other combination spills at either size (17-50 registers); lengths with a radix-5 / radix-7 stage stay with radix 4
#ifndef SMO_X_SEQ_HEAD_RADIX
#define SMO_X_SEQ_HEAD_RADIX ((only_2_and_3(L) && L <= 192) ? 8 : SMO_FFT_MAX_RADIX)
#endif
#ifndef SMO_X_SEQ_TAIL_RADIX
#define SMO_X_SEQ_TAIL_RADIX ((only_2_and_3(L) && L > 192) ? 8 : SMO_FFT_MAX_RADIX)
#endif
// Sequential adjoint x pass, n: the first n spectral items of B_f per thread are requested before the last forward stage of F1 instead of after
// F1's store loop: part of one global-memory round trip leaves the tile's critical path.  Registers decide how many: omega's grid values are
// live there, unlike in the second half where the running sum is requested at the same place.
#ifndef SMO_X_SEQ_PREFETCH
#define SMO_X_SEQ_PREFETCH (!only_2_and_3(L) ? 0 : L > 192 ? 3 : 2)     // lengths with a radix-5 / radix-7 stage have no registers to spare
#endif
// Sequential adjoint x pass, 1: those requests (B_f's spectra in the first half, the running sum in the second) are issued before the whole forward
// tail instead of before its last stage (G = 192: -1.3 %; at G = 384 the longer live ranges spill: +18 %)
// (parking part of omega's grid copy in the CU's idle LDS to make room for these at G = 384 was measured in round 4 and does not pay:
// profiles/r04_x384_levers.txt — the requested values compete with the radix-8 tail stages for the same registers, and those are worth more)
#ifndef SMO_X_SEQ_REQ_EARLY
#define SMO_X_SEQ_REQ_EARLY (only_2_and_3(L) && L <= 192)
#endif
// Sequential adjoint x pass, 1: the velocity is requested before omega's inverse transform (in flight during its LDS stages; omega's grid values
// are not live yet) instead of after it
#ifndef SMO_X_SEQ_U_EARLY
#define SMO_X_SEQ_U_EARLY only_2_and_3(L)
#endif
// Adjoint x pass of a frozen-velocity context (X_FUSED_ADJ_B: omega x U alone, the first half of the sequential pass): waves per SIMD it is
// built for.  Without B_f's prefetched spectra, the old running sum and a second set of grid values it needs the registers of the forward pass
// (DESIGN.md section 6f lists them per length), so it takes the forward pass's figure where the sequential pass has one of its own.
#ifndef SMO_X_ADJB_WAVES
#define SMO_X_ADJB_WAVES 4
#endif
// Write-through stores (st_cplx<true> below) on the hand-over streams of the time loop, one bit per stream:
//    1  Ty (work buffer or Ty-stack slot)     kd_y_pass<inv>
//    2  Tz                                    kd_y_pass<fwd>
//    4  the new state / snapshot              kd_z_forward, update modes
//    8  the next step's Tz                    kd_z_forward, NEXT tail
// A kernel ends with what its plain stores left dirty in the L2s still to be written back, and its successor starts behind that; a
// write-through store leaves nothing dirty.  It pays where a store instruction of a wave writes whole 128-byte lines, which these four do.
// (The x passes' streams — the EMF's spectrum / F1 and the running sum — were bits 16 and 32 and lost: a lane stores two adjacent 16-byte
// elements with two instructions, each half a line that only the L2 merges; +11 % and +5 % per gradient at 128^3, HISTORY.md.)
// SMO_KD_WT=0 in the environment: plain stores everywhere (KDynEnv).  G > 192 keeps plain stores (its own sweep: HISTORY.md).
#ifndef SMO_KD_WT
#define SMO_KD_WT (L <= 192 ? 15 : 0)
#endif
enum { WT_TY = 1, WT_TZ = 2, WT_STATE = 4, WT_NEXT = 8 };

// Workgroup shapes and per-length policies.  FFTs per workgroup are halved for the long transform (G = 384) so the LDS footprint per workgroup
// (<= 37-49 KB => 3-4 workgroups per CU) and the butterflies per thread stay what they are at G = 192.
template <int L> struct Shape {
    static constexpr int H = (L > 192) ? 2 : 1;
    static constexpr int ZNBT = SMO_Z_NBT, ZNT = SMO_Z_THREADS;          // z passes: row triples per workgroup, threads
    static constexpr bool ZHALF = (L >= SMO_Z_HALF_TW_MIN_L) && (L % 2 == 0);
    static constexpr int YZT = SMO_Y_ZT, YNT = 256;          // y pass: z columns per workgroup (512 threads: no change)
    static constexpr bool YHALF = (L >= SMO_Y_HALF_TW_MIN_L) && (L % 2 == 0);
    // forward x pass: (y,z) points per workgroup (12 / 6 FFTs; 128-B runs at G = 192)
    static constexpr int XT = 8 / H, XNT = SMO_X_FWD_NT, XRADIX = SMO_X_FWD_RADIX, XWAVES = SMO_X_WAVES;
    // sequential adjoint pass: one middle-section item (j, line pair) per thread — it keeps 9 complex grid values of omega per item in
    // registers, a second item per thread spills (G = 480: 320 items, 168 VGPRs + 241 spilled with 256 threads; 320 threads: none).  Hence
    // half tiles at G > 192 (40 KB, 168 VGPRs, three workgroups per CU; whole 128-byte lines there: 256 VGPRs + 91-159 spilled,
    // profiles/r04_x384_levers.txt) and XSNT >= XITEMS at every length.
    static constexpr int XTS = (L > 192) ? 4 : XT;
    static constexpr int XITEMS = (XTS / 2) * (L / 3);
    static constexpr int XSNT = XITEMS > SMO_X_SEQ_NT ? ((XITEMS + 63) / 64) * 64 : SMO_X_SEQ_NT;
    // the two-wave shape (SMO_X_SEQ_ITEMS = 2): half as many threads as items, two waves per SIMD; XSNT stays the one-item shape's figure
    static constexpr bool XS2 = (SMO_X_SEQ_ITEMS) == 2 && XITEMS == 256;
    static constexpr int XSNT2 = XITEMS / 2;
    static constexpr int xs_waves(int nt) { return nt < XITEMS ? 2 : SMO_X_SEQ_WAVES; }
    static constexpr int XSHEAD = SMO_X_SEQ_HEAD_RADIX, XSTAIL = SMO_X_SEQ_TAIL_RADIX, XSPRE = SMO_X_SEQ_PREFETCH;
    static constexpr bool XSREQ = SMO_X_SEQ_REQ_EARLY, XSUEARLY = SMO_X_SEQ_U_EARLY;
    // frozen-velocity adjoint pass: the sequential pass's tile and threads (one item per thread, whole 128-byte lines up to G = 192)
    static constexpr int XBT = XTS, XBNT = XSNT, XBWAVES = SMO_X_ADJB_WAVES;
    static constexpr int XTA = 4 / H, XANT = SMO_X_ADJ_NT;          // adjoint x pass: 12 / 6 FFTs of both field groups; 64 / 32-B runs, tiles grouped per XCD
    static constexpr int XTG = 16 / H, XGNT = 384;         // grid <-> spectrum only (setup / gradient output)
    static constexpr int WT = (SMO_KD_WT) & 15;            // write-through streams
    static constexpr bool wt(int stream) { return (WT & stream) != 0; }
};

struct Geom {
    int a;        // global number of kx modes (N/2)
    int al;       // local number of kx modes (a / world)
    int ix0;      // first global kx of this slab
    int m;        // ky / kz modes (N-1)
    int kmax;     // (N-1)/2
    int G;        // grid points per axis (3N/2)
    int Gzl;      // z planes the y / x passes of one launch see: the rank's slab G / world, or one of its `chunks` equal parts
    int Gzr;      // z planes per rank (G / world)
    int W;        // number of slabs
    int zg0;      // caller-layout grid vectors [3][G][G][Gzr]: first z plane of the chunk this launch works on
    size_t blk;   // slab-exchange layout: elements of one (chunk, peer) block (= field groups * 3 * al * m * Gzl)
    size_t cblk;  // elements between consecutive chunks (= W * 2 field groups * 3 * al * m * Gzl, whatever the number of groups in use,
                  // so that a chunk's region with one group lies inside its region with two)
    size_t typ;   // Ty: elements between consecutive (component, kx) planes (G * Gzl + padding; the padding keeps the x pass's 3a
                  // runs per tile off a power-of-two stride)
    int utile;    // x pass spectrum -> grid: 1 = write the tile-major layout of the internal U field (u_off), 0 = the flat X layout
    int tyl;      // layout of Ty: 0 = planes [c][kx][y][z] (+ padding per plane), 1 = z-block major [c][z/8][kx][y][z%8] (below)
    int ykx;      // y pass, z-block-major Ty: 1 = consecutive workgroups take consecutive kx (their G*128-byte blocks are adjacent)
    int act;      // members with their own horizon (Nh below): this launch belongs to a step that only members with Nh[b] >= act take part in
                  // (0: every member — setup, terminal condition, gradient output).  Sits in what was padding: the struct grows by Nh alone
    size_t tyk;   // z-block major: elements between consecutive kx blocks (8 G + one 128-byte line of padding)
    double Rm, dt;
    // members with their own horizon (smo_set_horizons): device table of B ints, member blockIdx.y runs Nh[blockIdx.y] <= n_iters steps, right-aligned
    // in the n_iters-step launch sequence.  Null: no horizons — nothing below reads a table then, nor `act`.  It sits in
    // front of the member strides, which every kernel reads for its pointers: the same 64 bytes of the kernel-argument segment.
    const int* Nh;
    // batched contexts (smo_config.batch = B): every launch has gridDim.y = B and workgroup row blockIdx.y works on member blockIdx.y, whose
    // copy of a per-member buffer starts this many elements after member 0's: coefficient fields (snapshots, G^, nu^), exchange buffers,
    // Ty-layout buffers (Ty, the running sum, the Ty cache), grid vectors (caller vectors, the U field).  Shared data (twiddles) is not strided.
    size_t mc, mz, mt, mg;
    // members with their own Rm (smo_create_members): device table of B doubles, member blockIdx.y takes entry blockIdx.y in place of Rm above.
    // Null for every context of smo_create / smo_create_multi, which read the kernel argument.  Written once at creation, never afterwards.
    const double* Rmb;
};

// Workgroup-uniform (blockIdx.y and kernel arguments alone): this member sits the step of this launch out.  Every kernel that uses it returns on
// it before its first barrier — behind its pointer set-up and the copy of the twiddle table, not as its first statement: a branch on a kernel
// argument at the very top makes every workgroup wait for that argument alone before it requests the others (one more round trip to the
// kernel-argument segment: + 0.2 us per kernel, 4.5 % of a 24^3 gradient).
// The empty statement below emits no instruction.  It names the geometry words every kernel's prologue computes with, so that they are
// requested together with Nh, in front of the branch: left alone, the compiler moves their loads behind it (they are first used there), and
// every workgroup of a context WITHOUT a table then waits for them a second time (+ 0.08 us per kernel at 24^3 even with the branch behind the
// twiddle copy).
__device__ __forceinline__ bool member_idle(const Geom& g) {
    asm volatile("" ::"s"(g.a), "s"(g.al), "s"(g.m), "s"(g.kmax), "s"(g.G), "s"(g.Gzl));
    return g.Nh && g.Nh[blockIdx.y] < g.act;
}

__device__ __forceinline__ int wrap_pos(int pos, const Geom& g) {      // position in the padded length-G spectrum -> stored index, -1 in the gap
    if (pos <= g.kmax) return pos;
    if (pos >= g.G - g.kmax) return pos - (g.G - g.m);
    return -1;
}
__device__ __forceinline__ double wavenumber(int idx, const Geom& g) { return (idx <= g.kmax) ? (double)idx : (double)(idx - g.m); }

// Tz in the slab-exchange layout [chunk (stride cblk)][peer][field group][3][al][m][Gzl] (the field-group offset is folded into the base pointer;
// chunk-major so that every chunk is one contiguous all_to_all_single, which lets the host pipeline the exchange of one chunk with
// the grid-side work on another):
// z side: the peer index is the z block of `pos`; rt = ixl * m + iy is the local (kx, ky) row
__device__ __forceinline__ size_t zs_off(int c, int rt, int pos, const Geom& g) {
    const size_t row = ((size_t)c * (g.al * g.m) + rt) * g.Gzl;
    if (g.Gzl == g.G) return row + pos;                                   // one slab, one chunk (uniform branch: no divisions)
    const int p = pos / g.Gzr, zl = pos - p * g.Gzr;
    const int k = zl / g.Gzl, zc = zl - k * g.Gzl;
    return (size_t)k * g.cblk + (size_t)p * g.blk + row + zc;
}
// caller-layout grid vector [3][G][G][Gzr]: offset of (c, x) at flat (y, z) index i of the chunk
__device__ __forceinline__ size_t grid_off(int c, int x, size_t i, const Geom& g) {
    const size_t y = i / g.Gzl;
    return (((size_t)c * g.G + x) * g.G + y) * g.Gzr + g.zg0 + (i - y * g.Gzl);
}
// y side (inside one chunk): the peer index is the kx block; offset of the (c, kx, iy = 0) row, z local
__device__ __forceinline__ size_t ys_row0(int c, int kx, const Geom& g) {
    const int q = kx / g.al;
    return (size_t)q * g.blk + ((size_t)c * g.al + (kx - q * g.al)) * ((size_t)g.m * g.Gzl);
}
// x pass: offset of mode kx (global) of component c, flat local (y,z) index i, in Ty[3][a][G*Gzl] (the plane layout; the run-time-length
// kernels of kdyn_any.hpp use only this one)
__device__ __forceinline__ size_t tx_off(int c, int kx, size_t i, const Geom& g) {
    return ((size_t)c * g.a + kx) * g.typ + i;
}
// Z-block-major Ty (round 3), Ty[c][z/8][kx][y][z%8], kx blocks G*8 + 8 elements apart.  In the plane layout a fused x-pass tile gathers one
// 64...128-byte run from each of 3a planes 16*G*Gzl bytes apart (2.4 MB at G = 384) and a y-pass workgroup G lines 16*Gzl bytes apart; here the
// x-pass runs of a tile lie G*128 + 128 bytes apart inside ONE window of a*(G*128 + 128) bytes per component (6.3 MB at G = 384; the extra line
// keeps them off one HBM channel, like the plane padding) and a y-pass workgroup (c, kx, 8 z columns) owns one contiguous G*128-byte block.
// tools/micro_patch_layout.hip, G = 384, same box: x pattern 4.95 -> 5.35 TB/s (tiles walked y-fastest inside a z block), y pattern 5.44 ->
// 5.63 TB/s (workgroups kx-fastest); 8x8 patches 5.36 / 5.22, row blocks 5.47 / 4.88; without the padding 4.17-4.33 (channel camping).
__device__ __forceinline__ size_t ty_off(int c, int kx, size_t i, const Geom& g) {      // any flat index i (one division: setup passes only)
    if (g.tyl == 0) return tx_off(c, kx, i, g);
    const size_t y = i / g.Gzl;
    const int z = (int)(i - y * g.Gzl);
    return (((size_t)c * (g.Gzl >> 3) + (z >> 3)) * g.a + kx) * g.tyk + y * 8 + (z & 7);
}
// the fused x passes: a tile of T <= 8 points starting at i0 (a multiple of T) lies inside one z block, so
//   offset(c, kx, i0 + e) = base + c * cs + kx * ks + e
struct XOrigin { size_t base, cs, ks; };
__device__ __forceinline__ XOrigin x_origin(size_t i0, const Geom& g) {
    if (g.tyl == 0) return XOrigin{i0, (size_t)g.a * g.typ, g.typ};
    const size_t y = i0 / g.Gzl;
    const int z0 = (int)(i0 - y * g.Gzl);
    return XOrigin{(size_t)(z0 >> 3) * g.a * g.tyk + y * 8 + (z0 & 7), (size_t)(g.Gzl >> 3) * g.a * g.tyk, g.tyk};
}

// The velocity field U is only ever read by the fused x passes, one (y,z) tile per workgroup, all x.  It is therefore kept
// tile-major, U[c][i/4][x][i%4] (i = flat local (y,z) index), so that a workgroup streams it as one contiguous run instead of
// G segments of 32-64 bytes (which cost 2-4x over-fetch of 128-byte lines).  Pairs (i, i+1) with i even never straddle a block.
constexpr int UT = 4;
__device__ __forceinline__ size_t u_off(int c, int x, size_t i, const Geom& g) {
    const size_t nt = ((size_t)g.G * g.Gzl) / UT;
    return (((size_t)c * nt + i / UT) * g.G + x) * UT + (i % UT);
}

// Streaming loads of the fused x passes.  At 128^3 a step hands ~1 GB from kernel to kernel (Ty, the EMF's spectrum, Tz) and those hand-overs can be
// served by the 256-MB cache behind the L2s — unless once-read streams displace them.  Two such streams are marked non-temporal:
//   the velocity tile (both passes): 170 MB per launch, the same every step            forward x pass 90.8 -> 80.4 us, adjoint 164.0 -> 159.7 us
//   the forward pass's input spectrum where a tile reads whole 128-byte lines (G <= 192) y<fwd> 35.3 -> 33.9 us; hurts with half-line tiles (G = 384)
// (the other once-per-step streams of the x and z passes were measured and gain nothing from the mark: profiles/r02_nt_streams.txt)
constexpr bool NT_VELOCITY = true, NT_FWD_SPECTRUM = true;
typedef double d2_t __attribute__((ext_vector_type(2)));
template <bool NTL = false> __device__ __forceinline__ cplx ld_cplx(const cplx* p) {       // (NTL = false: a plain load)
    if (NTL) { const d2_t v = __builtin_nontemporal_load(reinterpret_cast<const d2_t*>(p)); return mk(v.x, v.y); }
    return *p;
}
template <bool NTL> __device__ __forceinline__ cplx ld_pair(const double* q) {        // two consecutive grid values (16-byte aligned: even flat index)
    if (NTL) { const d2_t v = __builtin_nontemporal_load(reinterpret_cast<const d2_t*>(q)); return mk(v.x, v.y); }
    return mk(q[0], q[1]);
}
// Stores of the hand-over streams (SMO_KD_WT): element i of the stream that starts at `base`.  WT = false: the plain assignment.  WT = true: ONE
// 16-byte write-through (sc1) store — it goes to memory as it is issued and leaves no dirty line in the L2 for the end of the kernel.  It is a
// buffer store: the compiler sees it and schedules it (an asm statement with a memory clobber would pin the early requests of the x passes
// in place).  `base` is workgroup-uniform (a kernel argument + the member's offset), the byte offset 16 i is below 4 GB for every buffer a
// launch writes (the largest, one field group of Ty at G = 480, is 1.8 GB), and the resource's range is left at the maximum: nothing is
// clipped, so a wrong index lands where a plain store's would and SMO_GUARD sees it.  Always whole 16-byte elements — narrower write-through
// stores cost 2.7x and more per byte.
typedef unsigned u4_t __attribute__((ext_vector_type(4)));
template <bool WT> __device__ __forceinline__ void st_cplx(cplx* base, size_t i, cplx v) {
    if constexpr (WT) {
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, -1, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4_t, v), rsrc, (int)(unsigned)(i * 16), 0, 16 /* sc1 */);
    } else {
        base[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------
// z pass, inverse (coefficients -> Tz), rows contiguous.  NBT (ix,iy) row triples per workgroup.
// ---------------------------------------------------------------------------------------------------------
enum { ZI_PLAIN = 0, ZI_CURL = 1, ZI_SCALE = 2 };     // load the field | load i k x field | load dt*alpha(k)*field

// Tile of the z passes: one row per transform (lanes run along a row: the global accesses are the contiguous ones), element (b, pos) at
// b * L + pos.  Row-major stays: a swizzled tile removes bank conflicts of the first two Stockham stages and no time (profiles/r04_z_tile_swizzle.txt).
template <int L> struct ZIx {
    __device__ __forceinline__ int operator()(int b, int pos) const { return b * L + pos; }
};

template <int L, int MODE, int NBT, int NT>
__global__ __launch_bounds__(NT) void kd_z_inverse(const cplx* __restrict__ in, cplx* __restrict__ out, const cplx* __restrict__ tw_g,
                                                   Geom g) {
    constexpr int NB = 3 * NBT;
    constexpr ZIx<L> ix{};
    __shared__ cplx buf[NB * L];
    in += blockIdx.y * g.mc;                                // batch member (Geom::mc / mz)
    out += blockIdx.y * g.mz;
    double Rm = g.Rm;                                       // ... and its own Rm where the context has a table (Geom::Rmb): workgroup-uniform
    if constexpr (MODE == ZI_SCALE) { if (g.Rmb) Rm = g.Rmb[blockIdx.y]; }
    constexpr bool HALF = Shape<L>::ZHALF;                  // half twiddle table (SMO_Z_HALF_TW_MIN_L)
    constexpr int NTW = HALF ? L / 2 : L;
    __shared__ cplx tw_s[NTW];
    const int tid = threadIdx.x;
    for (int i = tid; i < NTW; i += NT) tw_s[i] = tw_g[i];
    if (member_idle(g)) return;                             // (a member whose horizon has not begun / is over: Geom::Nh)
    __syncthreads();
    using TWT = typename std::conditional<HALF, HalfTwiddles, const cplx*>::type;
    TWT tw;
    if constexpr (HALF) tw = HalfTwiddles{tw_s, L / 2};
    else tw = tw_s;
    const int nrt = g.al * g.m;
    const int rt0 = blockIdx.x * NBT;
    const size_t cs = (size_t)nrt * g.m;
    auto ld0 = [&](int b, int pos) -> cplx {
        const int tt = b / 3, c = b - 3 * tt, rt = rt0 + tt;
        const int idx = wrap_pos(pos, g);
        if (rt >= nrt || idx < 0) return mk(0, 0);
        const size_t e = (size_t)rt * g.m + idx;
        if (MODE == ZI_PLAIN) return in[c * cs + e];
        const int ixl = rt / g.m, iy = rt - ixl * g.m;
        const double k[3] = {(double)(g.ix0 + ixl), wavenumber(iy, g), wavenumber(idx, g)};
        if (MODE == ZI_SCALE) {
            const double s = g.dt * (1.0 / g.dt + 0.5 * (k[0] * k[0] + k[1] * k[1] + k[2] * k[2]) / Rm);
            return s * in[c * cs + e];
        }
        const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
        cplx v1 = in[c1 * cs + e], v2 = in[c2 * cs + e];
        return mul_i(mk(k[c1] * v2.re - k[c2] * v1.re, k[c1] * v2.im - k[c2] * v1.im));      // (i k x V)_c
    };
    auto stN = [&](int b, int pos, cplx v) {
        const int tt = b / 3, c = b - 3 * tt, rt = rt0 + tt;
        if (rt < nrt) out[zs_off(c, rt, pos, g)] = v;
    };
    if (MODE == ZI_CURL) {
        // every component feeds two components of the curl: read the rows once, coalesced, into the tile and form i k x V from there
        // (loading them twice from global memory cost 20 % at G = 192 and 35 % at G = 384)
        for (int t = tid; t < NB * g.m; t += NT) {
            const int b = t / g.m, idx = t - b * g.m, tt = b / 3, c = b - 3 * tt, rt = rt0 + tt;
            const int pos = (idx <= g.kmax) ? idx : idx + (g.G - g.m);
            buf[ix(b, pos)] = (rt < nrt) ? in[c * cs + (size_t)rt * g.m + idx] : mk(0, 0);
        }
        __syncthreads();
        auto ldc = [&](int b, int pos) -> cplx {
            const int tt = b / 3, c = b - 3 * tt, rt = rt0 + tt;
            const int idx = wrap_pos(pos, g);
            if (rt >= nrt || idx < 0) return mk(0, 0);
            const int ixl = rt / g.m, iy = rt - ixl * g.m;
            const double k[3] = {(double)(g.ix0 + ixl), wavenumber(iy, g), wavenumber(idx, g)};
            const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            const cplx v1 = buf[ix(tt * 3 + c1, pos)], v2 = buf[ix(tt * 3 + c2, pos)];
            return mul_i(mk(k[c1] * v2.re - k[c2] * v1.re, k[c1] * v2.im - k[c2] * v1.im));      // (i k x V)_c
        };
        fft_inplace_ix<L, true, NB, NT, false, true, false>(buf, ix, tw, tid, ldc, stN);
        return;
    }
    fft_inplace_ix<L, true, NB, NT, false, false, false>(buf, ix, tw, tid, ld0, stN);
}

// ---------------------------------------------------------------------------------------------------------
// z pass, forward (Tz -> coefficients), with the per-mode time-step fused in
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cnab_mode(const double k[3], double k2, double alpha, double beta, const cplx V0[3], const cplx F[3],
                                          cplx V1[3]) {
    if (k2 == 0.0) {                                    // algebraic rows under CNAB1: X1 = -X0
        for (int c = 0; c < 3; ++c) V1[c] = mk(-V0[c].re, -V0[c].im);
        return;
    }
    cplx r[3];
    for (int c = 0; c < 3; ++c) r[c] = mk(beta * V0[c].re + F[c].re, beta * V0[c].im + F[c].im);
    const double ik2 = 1.0 / k2;
    const cplx kr = mk((k[0] * r[0].re + k[1] * r[1].re + k[2] * r[2].re) * ik2, (k[0] * r[0].im + k[1] * r[1].im + k[2] * r[2].im) * ik2);
    const cplx kv = mk((k[0] * V0[0].re + k[1] * V0[1].re + k[2] * V0[2].re) * ik2,
                       (k[0] * V0[0].im + k[1] * V0[1].im + k[2] * V0[2].im) * ik2);
    for (int c = 0; c < 3; ++c)
        V1[c] = mk((r[c].re - k[c] * kr.re) / alpha - k[c] * kv.re, (r[c].im - k[c] * kr.im) / alpha - k[c] * kv.im);
}

enum { ZF_PLAIN = 0, ZF_FWD_UPDATE = 1, ZF_ADJ_UPDATE = 2, ZF_NU = 3 };

// ZF_PLAIN: truncated spectrum;  ZF_FWD_UPDATE: B^_{n+1};  ZF_ADJ_UPDATE: G^ update with forcing F1 = F[(curl G) x U] (minus 2 B_f if
// integrated);  ZF_NU: nu^ = -dt P(F[sum_n (curl G_n) x B_n]) from the accumulated product (see the fused adjoint x pass)
// NEXT: the z pass that opens the following time step works on the very rows this kernel has just updated, so it can run here, on the
// tile, instead of re-reading the new state in a kernel of its own: NX_PLAIN = inverse z pass of the new state (forward solve),
// NX_CURL = inverse z pass of i k x (new state) (adjoint solve).  The result goes where the input came from (the z-side exchange
// buffer, same layout), which is safe because a workgroup owns its rows.
enum { NX_NONE = 0, NX_PLAIN = 1, NX_CURL = 2 };
template <int L, int MODE, int NEXT, int NBT, int NT, int WT = 0>         // WT: write-through streams of this launch (WT_STATE | WT_NEXT)
__global__ __launch_bounds__(NT) void kd_z_forward(const cplx* inA, cplx* out0, const cplx* state0 /* may alias out0 */,
                                                   const cplx* snap, const cplx* __restrict__ tw_g, Geom g, double scale, int integrated,
                                                   cplx* next_out /* may alias inA */) {
    constexpr int NB = 3 * NBT;
    constexpr ZIx<L> ix{};
    __shared__ cplx buf[NB * L];
    inA += blockIdx.y * g.mz;                               // batch member (Geom::mc / mz); the pointers a mode does not use stay as passed
    out0 += blockIdx.y * g.mc;
    if constexpr (MODE == ZF_FWD_UPDATE || MODE == ZF_ADJ_UPDATE) state0 += blockIdx.y * g.mc;
    if constexpr (MODE == ZF_ADJ_UPDATE) snap += blockIdx.y * g.mc;
    if constexpr (NEXT != NX_NONE) next_out += blockIdx.y * g.mz;
    double Rm = g.Rm;                                       // ... and its own Rm where the context has a table (Geom::Rmb): workgroup-uniform
    if constexpr (MODE == ZF_FWD_UPDATE || MODE == ZF_ADJ_UPDATE) { if (g.Rmb) Rm = g.Rmb[blockIdx.y]; }
    constexpr bool HALF = Shape<L>::ZHALF;                  // half twiddle table (SMO_Z_HALF_TW_MIN_L)
    constexpr int NTW = HALF ? L / 2 : L;
    __shared__ cplx tw_s[NTW];
    const int tid = threadIdx.x;
    for (int i = tid; i < NTW; i += NT) tw_s[i] = tw_g[i];
    // members with their own horizon (Geom::Nh).  Adjoint update: a member whose sweep is over leaves G^ as it is.  Forward update: a member whose
    // horizon has not begun hands its state on unchanged (snap(n+1) = snap(n): checkpoints, replayed windows and the two-slot stack then need no
    // special case) and still runs the NEXT tail on it, so that its first own step finds what a fused predecessor leaves.
    bool idle = false;
    if constexpr (MODE == ZF_ADJ_UPDATE) { if (member_idle(g)) return; }
    if constexpr (MODE == ZF_FWD_UPDATE) idle = member_idle(g);
    __syncthreads();
    using TWT = typename std::conditional<HALF, HalfTwiddles, const cplx*>::type;
    TWT tw;
    if constexpr (HALF) tw = HalfTwiddles{tw_s, L / 2};
    else tw = tw_s;
    const int nrt = g.al * g.m;
    const int rt0 = blockIdx.x * NBT;
    const size_t cs = (size_t)nrt * g.m;
    // b = tt * 3 + c
    auto ld0 = [&](int b, int pos) -> cplx {
        const int c = b % 3, tt = b / 3, rt = rt0 + tt;
        if (rt >= nrt) return mk(0, 0);
        return inA[zs_off(c, rt, pos, g)];
    };
    if (MODE == ZF_PLAIN) {
        auto stN = [&](int b, int pos, cplx v) {
            const int c = b % 3, tt = b / 3, rt = rt0 + tt;
            const int idx = wrap_pos(pos, g);
            if (rt < nrt && idx >= 0) out0[c * cs + (size_t)rt * g.m + idx] = scale * v;
        };
        fft_inplace_ix<L, false, NB, NT, false, false, false>(buf, ix, tw, tid, ld0, stN);
        return;
    }
    if (!idle) fft_inplace_ix<L, false, NB, NT, false, false, true>(buf, ix, tw, tid, ld0, [&](int b, int pos, cplx v) { buf[ix(b, pos)] = v; });
    __syncthreads();
    // per-mode update: thread <-> (tt, iz), iz fastest
    for (int t = tid; t < NBT * g.m; t += NT) {
        const int tt = t / g.m, iz = t - tt * g.m, rt = rt0 + tt;
        if (rt >= nrt) continue;
        const int ixl = rt / g.m, iy = rt - ixl * g.m;
        const int pos = (iz <= g.kmax) ? iz : iz + (g.G - g.m);
        const double k[3] = {(double)(g.ix0 + ixl), wavenumber(iy, g), wavenumber(iz, g)};
        const double k2 = k[0] * k[0] + k[1] * k[1] + k[2] * k[2];
        const double D = k2 / Rm, alpha = 1.0 / g.dt + 0.5 * D, beta = 1.0 / g.dt - 0.5 * D;
        const size_t e = (size_t)rt * g.m + iz;
        cplx E[3], V0[3], V1[3];
        for (int c = 0; c < 3; ++c) E[c] = scale * buf[ix(tt * 3 + c, pos)];
        if (MODE == ZF_NU) {
            if (k2 == 0.0) {
                for (int c = 0; c < 3; ++c) V1[c] = mk(0, 0);
            } else {
                const double ik2 = 1.0 / k2;
                const cplx kf = mk((k[0] * E[0].re + k[1] * E[1].re + k[2] * E[2].re) * ik2, (k[0] * E[0].im + k[1] * E[1].im + k[2] * E[2].im) * ik2);
                for (int c = 0; c < 3; ++c) V1[c] = mk(-g.dt * (E[c].re - k[c] * kf.re), -g.dt * (E[c].im - k[c] * kf.im));
            }
            for (int c = 0; c < 3; ++c) out0[c * cs + e] = V1[c];
            continue;
        }
        for (int c = 0; c < 3; ++c) V0[c] = state0[c * cs + e];
        if (MODE == ZF_FWD_UPDATE) {
            cplx F[3];                                  // N^ = i k x E^
            for (int c = 0; c < 3; ++c) {
                const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                F[c] = mul_i(mk(k[c1] * E[c2].re - k[c2] * E[c1].re, k[c1] * E[c2].im - k[c2] * E[c1].im));
            }
            if (idle) { for (int c = 0; c < 3; ++c) V1[c] = V0[c]; }      // (the tile holds nothing of this member: E, F are not used)
            else cnab_mode(k, k2, alpha, beta, V0, F, V1);
        } else {
            if (integrated)
                for (int c = 0; c < 3; ++c) { cplx bf = snap[c * cs + e]; E[c] = mk(E[c].re - 2.0 * bf.re, E[c].im - 2.0 * bf.im); }
            cnab_mode(k, k2, alpha, beta, V0, E, V1);
        }
        for (int c = 0; c < 3; ++c) st_cplx<(WT & WT_STATE) != 0>(out0, c * cs + e, V1[c]);
        if (NEXT != NX_NONE) {                          // the new state (or its curl) replaces the spectrum in the tile
            for (int c = 0; c < 3; ++c) {
                const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                buf[ix(tt * 3 + c, pos)] = (NEXT == NX_PLAIN) ? V1[c]
                    : mul_i(mk(k[c1] * V1[c2].re - k[c2] * V1[c1].re, k[c1] * V1[c2].im - k[c2] * V1[c1].im));
            }
        }
    }
    if (NEXT != NX_NONE) {
        const int gap = g.G - g.m;                      // zero padding between the positive and the negative wavenumbers
        for (int t = tid; t < NB * gap; t += NT) {
            const int b = t / gap, q = t - b * gap;
            buf[ix(b, g.kmax + 1 + q)] = mk(0, 0);
        }
        __syncthreads();
        fft_inplace_ix<L, true, NB, NT, false, true, false>(buf, ix, tw, tid, [&](int b, int pos) { return buf[ix(b, pos)]; },
                                                         [&](int b, int pos, cplx v) {
                                                             const int c = b % 3, tt = b / 3, rt = rt0 + tt;
                                                             if (rt < nrt) st_cplx<(WT & WT_NEXT) != 0>(next_out, zs_off(c, rt, pos, g), v);
                                                         });
    }
}

// ---------------------------------------------------------------------------------------------------------
// y pass (strided): Tz (slab-exchange layout, all kx, local z) <-> Ty[3][a][G][Gzl]; ZT consecutive z per workgroup
// ---------------------------------------------------------------------------------------------------------
template <int L, bool INV, int ZT, int NT, bool WT = false>              // WT: write-through stores (WT_TY / WT_TZ)
__global__ __launch_bounds__(NT) void kd_y_pass(const cplx* __restrict__ in, cplx* __restrict__ out, const cplx* __restrict__ tw_g, Geom g) {
    // position-major tile (PosMajor, fft_lds.hpp): the ZT columns of a tile interleaved, every stage access of a wave is one contiguous
    // run (model: G = 192 reads 2x -> 1x, G = 384 3x -> 1x conflict cycles against rows of L + 1)
    constexpr PosMajor<ZT> ix{};
    // the z-block-major Ty addressing below (trow, tys = 8) is written for tiles that lie inside one block of 8 z columns
    static_assert(ZT <= 8 && 8 % ZT == 0, "kd_y_pass: SMO_Y_ZT must divide 8 (z-block-major Ty)");
    __shared__ cplx buf[ZT * L];
    in += blockIdx.y * (INV ? g.mz : g.mt);                 // batch member (Geom::mz / mt)
    out += blockIdx.y * (INV ? g.mt : g.mz);
    constexpr bool HALF = Shape<L>::YHALF;                  // half twiddle table (SMO_Y_HALF_TW_MIN_L)
    constexpr int NTW = HALF ? L / 2 : L;
    __shared__ cplx tw_s[NTW];
    const int tid = threadIdx.x;
    for (int i = tid; i < NTW; i += NT) tw_s[i] = tw_g[i];
    if (member_idle(g)) return;                             // (a member whose horizon has not begun / is over: Geom::Nh)
    __syncthreads();
    using TWT = typename std::conditional<HALF, HalfTwiddles, const cplx*>::type;
    TWT tw;
    if constexpr (HALF) tw = HalfTwiddles{tw_s, L / 2};
    else tw = tw_s;
    const int ntile = (g.Gzl + ZT - 1) / ZT;
    int c, kx, z0;
    if (g.tyl && g.ykx) {                       // consecutive workgroups: consecutive kx of one (c, z tile) — adjacent blocks of Ty
        kx = blockIdx.x % g.a;
        const int r = blockIdx.x / g.a;
        c = r / ntile; z0 = (r - c * ntile) * ZT;
    } else {
        const int o = blockIdx.x / ntile;       // o = c * a + kx
        z0 = (blockIdx.x - o * ntile) * ZT;
        c = o / g.a; kx = o - c * g.a;
    }
    const size_t zrow = ys_row0(c, kx, g) + z0;                               // + idx * Gzl + b
    // Ty side: + y * tys + b
    const size_t trow = g.tyl ? (((size_t)c * (g.Gzl >> 3) + (z0 >> 3)) * g.a + kx) * g.tyk + (z0 & 7) : ((size_t)c * g.a + kx) * g.typ + z0;
    const size_t tys = g.tyl ? 8 : (size_t)g.Gzl;
    if (INV) {
        auto ld0 = [&](int b, int pos) -> cplx {
            const int idx = wrap_pos(pos, g);
            if (idx < 0 || z0 + b >= g.Gzl) return mk(0, 0);
            return in[zrow + (size_t)idx * g.Gzl + b];
        };
        auto stN = [&](int b, int pos, cplx v) {
            if (z0 + b < g.Gzl) st_cplx<WT>(out, trow + (size_t)pos * tys + b, v);
        };
        fft_inplace_ix<L, true, ZT, NT, true, false, false>(buf, ix, tw, tid, ld0, stN);
    } else {
        auto ld0 = [&](int b, int pos) -> cplx {
            if (z0 + b >= g.Gzl) return mk(0, 0);
            return in[trow + (size_t)pos * tys + b];
        };
        auto stN = [&](int b, int pos, cplx v) {
            const int idx = wrap_pos(pos, g);
            if (idx >= 0 && z0 + b < g.Gzl) st_cplx<WT>(out, zrow + (size_t)idx * g.Gzl + b, v);
        };
        fft_inplace_ix<L, false, ZT, NT, true, false, false>(buf, ix, tw, tid, ld0, stN);
    }
}

// ---------------------------------------------------------------------------------------------------------
// x pass (strided, real <-> Hermitian half spectrum), two real lines per complex FFT, T flat (y,z) points per
// workgroup.  Modes: spectrum -> grid; grid -> spectrum; fused  spectrum -> grid product(s) -> spectrum.
// ---------------------------------------------------------------------------------------------------------
enum { X_TO_GRID = 0, X_FROM_GRID = 1, X_FUSED_FWD = 2, X_FUSED_ADJ = 3, X_FUSED_ADJ_SEQ = 4,
       X_FUSED_ADJ_B = 5 };      // the adjoint pass of a context whose velocity is frozen (smo_create_frozen_u): omega x U alone

// Row padding of the x pass's LDS tile (complex elements).  Lanes run over the NB transforms first, then over consecutive positions:
// element (b, pos) starts at bank group (pad * b + pos) mod 16, and a 64-lane 16-byte access is conflict-free when each of the 16
// groups gets 4 lanes, i.e. when the NB ranges [pad * b, pad * b + 64/NB) tile the line: pad ~ 64 / NB.
constexpr int x_ld_pad(int NB) { return NB == 12 ? 5 : (NB == 6 ? 10 : 1); }
// Layout of the fused x passes' tile: position-major (the NB transforms of a tile interleaved, see PosMajor in fft_lds.hpp) — every
// stage read of a wave is one contiguous run, no row padding needed.  The two unfused modes keep the row-per-transform layout.
template <int L, int NB, bool FUSED> struct XLayout {
    static constexpr bool PM = FUSED;
    static constexpr int LD = L + x_ld_pad(NB);
    static constexpr int ELEMS = PM ? NB * L : NB * LD;
    __device__ __forceinline__ int operator()(int b, int pos) const { return PM ? pos * NB + b : b * LD + pos; }
};

// spectra of the x pass: field groups A / B are read from in* and written to out* (same layout; in == out means in place)
struct XSpec {
    const cplx* inA;
    const cplx* inB;
    cplx* outA;
    cplx* outB;
};

template <int L, int MODE, int T, int NT, class TW>
__device__ __forceinline__ void x_tile(const XSpec& sp, const double* __restrict__ gridU, double* gridOut, const Geom& g,
                                       cplx* buf, const TW tw, const size_t i0, const int tid) {
    constexpr int NF = (MODE == X_FUSED_ADJ) ? 2 : 1;
    constexpr int HP = T / 2;                       // line pairs
    constexpr int NB = NF * 3 * HP;
    constexpr XLayout<L, NB, (MODE == X_FUSED_FWD || MODE == X_FUSED_ADJ)> ix{};
    const size_t plane = (size_t)g.G * g.Gzl;       // local (y,z) points
    // b = (f*3 + c)*HP + p
    auto line_ok = [&](int p) { return i0 + 2 * p < plane; };      // plane is even, T is even: pairs never straddle the end
    // offset in Ty of (component c, mode kx, line pair p of this tile): tiles of up to 8 points lie inside one z block of either layout
    const XOrigin xo = x_origin(i0, g);
    auto spec_off = [&](int c, int kx, int p) -> size_t {
        if constexpr (T <= 8) return xo.base + c * xo.cs + kx * xo.ks + 2 * p;
        else return ty_off(c, kx, i0 + 2 * p, g);
    };

    // -- load (spectrum, Hermitian extension) or (grid, two real lines) ------------------------------------------
    auto ld_spec = [&](int b, int pos) -> cplx {
        const int p = b % HP, fc = b / HP, c = fc % 3, f = fc / 3;
        if (!line_ok(p)) return mk(0, 0);
        const cplx* src = (f == 0) ? sp.inA : sp.inB;
        int kx; bool cj;
        if (pos < g.a) { kx = pos; cj = false; }
        else if (pos > g.G - g.a) { kx = g.G - pos; cj = true; }
        else return mk(0, 0);
        const size_t off = spec_off(c, kx, p);
        cplx X1 = src[off], X2 = src[off + 1];
        if (kx == 0) return mk(X1.re, X2.re);                       // c2r ignores the imaginary part of kx = 0
        if (cj) return mk(X1.re + X2.im, X2.re - X1.im);            // conj(X1) + i conj(X2)
        return mk(X1.re - X2.im, X1.im + X2.re);                    // X1 + i X2
    };
    auto ld_grid = [&](int b, int pos) -> cplx {
        const int p = b % HP, c = b / HP;
        if (!line_ok(p)) return mk(0, 0);
        const double* q = gridU + grid_off(c, pos, i0 + 2 * p, g);
        return mk(q[0], q[1]);
    };
    auto st_buf = [&](int b, int pos, cplx v) { buf[ix(b, pos)] = v; };

    if (MODE == X_TO_GRID) {
        fft_inplace_ix<L, true, NB, NT, true, false, false>(buf, ix, tw, tid, ld_spec, [&](int b, int pos, cplx v) {
            const int p = b % HP, c = b / HP;
            if (line_ok(p)) {
                double* q = gridOut + (g.utile ? u_off(c, pos, i0 + 2 * p, g) : grid_off(c, pos, i0 + 2 * p, g));
                q[0] = v.re; q[1] = v.im;
            }
        });
        return;
    }
    constexpr bool ACC = (MODE == X_FUSED_ADJ);
    constexpr int SCNT = ((L / 3) * NF * 3 * HP + NT - 1) / NT;        // items per thread of the final split / store loop
    cplx old_sum[ACC ? SCNT : 1][2];
    if (MODE == X_FROM_GRID) {
        fft_inplace_ix<L, false, NB, NT, true, false, true>(buf, ix, tw, tid, ld_grid, st_buf);
    } else {
        // The middle of the pass runs in registers.  G = 3N/2, so the inverse transform (radix order 4..4[2]3) ENDS with a radix-3
        // butterfly over x = j, j + a, j + 2a (a = L/3), and the forward transform, taken in the order 3 4..4[2], BEGINS with a radix-3
        // butterfly over the same three points.  A thread that owns (j, line pair p) for every component therefore does: last inverse
        // butterflies -> cross product(s) at its three grid points -> first forward butterflies (+ twiddles), touching the LDS once
        // (read j + k a, write 3 j + k) with one barrier in between, instead of three round trips and three barriers.  The velocity is
        // requested before that barrier and arrives while the others finish reading.  Item = (j, p), p fastest.
        // Radix policy: Shape<L> (SMO_X_FWD_RADIX; X_FUSED_ADJ follows the sequential adjoint pass)
        using S = Shape<L>;
        constexpr int XRH = (MODE == X_FUSED_FWD) ? S::XRADIX : (MODE == X_FUSED_ADJ ? S::XSHEAD : SMO_FFT_MAX_RADIX);      // inverse head
        constexpr int XRT = (MODE == X_FUSED_FWD) ? S::XRADIX : (MODE == X_FUSED_ADJ ? S::XSTAIL : SMO_FFT_MAX_RADIX);      // forward tail
        static_assert(last_radix<L, XRH>() == 3, "G = 3N/2: the last Stockham stage is radix 3");
        // every stored mode feeds two positions of the Hermitian-extended line (kx and G - kx): read it once, coalesced (p fastest: one
        // 128-byte run per (component, kx)), and write both into the tile; the first butterfly stage then works LDS -> LDS
        for (int t = tid; t < (L / 3) * NF * 3 * HP; t += NT) {
            const int p = t % HP, r = t / HP, fc = r % (NF * 3), kx = r / (NF * 3), c = fc % 3, f = fc / 3;
            cplx X1 = mk(0, 0), X2 = mk(0, 0);
            if (line_ok(p)) {
                const cplx* src = ((f == 0) ? sp.inA : sp.inB) + spec_off(c, kx, p);
                // (forward pass, tiles of whole 128-byte lines: its input spectrum is dead once read — non-temporal, so that the hit does not renew it)
                constexpr bool NTIN = NT_FWD_SPECTRUM && MODE == X_FUSED_FWD && T >= 8;
                X1 = ld_cplx<NTIN>(src); X2 = ld_cplx<NTIN>(src + 1);
            }
            const int b = fc * HP + p;
            if (kx == 0) buf[ix(b, 0)] = mk(X1.re, X2.re);                    // c2r ignores the imaginary part of kx = 0
            else {
                buf[ix(b, kx)] = mk(X1.re - X2.im, X1.im + X2.re);            // X1 + i X2
                buf[ix(b, L - kx)] = mk(X1.re + X2.im, X2.re - X1.im);        // conj(X1) + i conj(X2)
            }
        }
        constexpr int S3 = L / 3;
        constexpr int ICNT = (HP * S3 + NT - 1) / NT;
        cplx U0[3][3];                              // velocity at the first item's points, [k][component]
        // forward pass: the velocity is requested before the inverse transform's LDS stages instead of after them
        constexpr bool UEARLY = MODE == X_FUSED_FWD;
        if (UEARLY) {
            const int j = tid / HP, p = tid - j * HP;
            if (tid < HP * S3 && line_ok(p))
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    for (int c = 0; c < 3; ++c) U0[k][c] = ld_pair<NT_VELOCITY>(gridU + u_off(c, j + S3 * k, i0 + 2 * p, g));
        }
        __syncthreads();
        fft_inplace_head_r<XRH, L, true, NB, NT, true, true>(buf, ix, tw, tid, [&](int b, int pos) -> cplx {
            return (pos >= L / 3 && pos <= L - L / 3) ? mk(0, 0) : buf[ix(b, pos)];        // the zero padding is never stored
        });
        cplx Win[ICNT][NF][3][3];                   // [item][field group][component][k]: inputs of the last inverse stage
#pragma unroll
        for (int i = 0; i < ICNT; ++i) {
            const int t = tid + i * NT, j = t / HP, p = t - j * HP;
            if (t < HP * S3 && line_ok(p)) {
#pragma unroll
                for (int f = 0; f < NF; ++f)
                    for (int c = 0; c < 3; ++c)
                        for (int k = 0; k < 3; ++k) Win[i][f][c][k] = buf[ix((f * 3 + c) * HP + p, j + S3 * k)];
                if (i == 0 && !UEARLY)
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        for (int c = 0; c < 3; ++c) {
                            U0[k][c] = ld_pair<NT_VELOCITY>(gridU + u_off(c, j + S3 * k, i0 + 2 * p, g));
                        }
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ICNT; ++i) {
            const int t = tid + i * NT, j = t / HP, p = t - j * HP;
            if (t >= HP * S3 || !line_ok(p)) continue;
            cplx U[3][3], W[3][3];                  // [x = j + k a][component]; .re / .im = the two real lines of the pair
#pragma unroll
            for (int k = 0; k < 3; ++k)
                for (int c = 0; c < 3; ++c) {
                    if (i == 0) U[k][c] = U0[k][c];
                    else U[k][c] = ld_pair<NT_VELOCITY>(gridU + u_off(c, j + S3 * k, i0 + 2 * p, g));
                }
            auto last_stage = [&](int f, cplx (&out)[3][3]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    cplx v[3];
                    for (int k = 0; k < 3; ++k) v[k] = Win[i][f][c][k];
                    Butterfly<3, true>::run(v);
                    for (int k = 0; k < 3; ++k) out[k][c] = v[k];
                }
            };
            auto cross_to = [&](int f, const cplx (&X)[3][3], const cplx (&Y)[3][3]) {       // field group f <- first forward stage of X x Y
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
                    cplx v[3];
                    for (int k = 0; k < 3; ++k)
                        v[k] = mk(X[k][c1].re * Y[k][c2].re - X[k][c2].re * Y[k][c1].re, X[k][c1].im * Y[k][c2].im - X[k][c2].im * Y[k][c1].im);
                    Butterfly<3, false>::run(v);
                    const int b = (f * 3 + c) * HP + p;
                    buf[ix(b, 3 * j)] = v[0];
                    buf[ix(b, 3 * j + 1)] = twmul<false>(v[1], tw[j]);
                    buf[ix(b, 3 * j + 2)] = twmul<false>(v[2], tw[2 * j]);
                }
            };
            last_stage(0, W);
            if (MODE == X_FUSED_FWD) {
                cross_to(0, U, W);                  // EMF = U x B
            } else {
                cross_to(0, W, U);                  // F1 = omega x U
                last_stage(1, U);                   // B_f takes the velocity's registers
                cross_to(1, W, U);                  // F2' = omega x B_f
            }
        }
        __syncthreads();
        // remaining forward stages (sub-length a, stride 3); group B of the adjoint pass is a running sum: its old values are requested
        // before the last stage
        InplaceTail<L, L / 3, 3, false, NB, NT, true, true, XRT>::run_ix(buf, ix, tid, tw, st_buf, [&]() {
            if (ACC) {
#pragma unroll
                for (int i = 0; i < SCNT; ++i) {
                    const int t = tid + i * NT, p = t % HP, r = t / HP, fc = r % (NF * 3), kx = r / (NF * 3);
                    if (t < (L / 3) * NF * 3 * HP && fc >= 3 && line_ok(p)) {
                        const cplx* q = sp.outB + spec_off(fc - 3, kx, p);
                        old_sum[i][0] = q[0]; old_sum[i][1] = q[1];
                    }
                }
            }
        });
    }
    __syncthreads();
    // split the two real lines' spectra and store kx = 0..a-1 (a = L/3); item = ((kx*NF*3 + fc)*HP + p), p fastest
#pragma unroll
    for (int i = 0; i < SCNT; ++i) {
        const int t = tid + i * NT;
        if (t >= (L / 3) * NF * 3 * HP) break;
        const int p = t % HP, r = t / HP, fc = r % (NF * 3), kx = r / (NF * 3);
        if (!line_ok(p)) continue;
        const int c = fc % 3, f = fc / 3;
        const cplx Zk = buf[ix(fc * HP + p, kx)];
        const cplx Zm = conj(buf[ix(fc * HP + p, (kx == 0) ? 0 : L - kx)]);
        cplx* dst = ((f == 0) ? sp.outA : sp.outB) + spec_off(c, kx, p);
        cplx v0 = 0.5 * (Zk + Zm), v1 = mul_mi(0.5 * (Zk - Zm));
        if (ACC && f == 1) { v0 = v0 + old_sum[i][0]; v1 = v1 + old_sum[i][1]; }
        dst[0] = v0;
        dst[1] = v1;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Adjoint x pass, field groups ONE AFTER THE OTHER through the tile buffer (X_FUSED_ADJ_SEQ).  The pass needs omega = curl G and B_f on
// the grid at the same points; X_FUSED_ADJ transforms both at once (6 * HP transforms in the tile), which at a given LDS footprint halves
// the (y,z) points per tile: 64-byte runs of the spectra at G = 192, 32-byte runs at G = 384 — and the access pattern itself then caps the
// pass (tools/micro_gather.hip: a bare copy with that pattern reaches 5.1 / 3.6 TB/s, with runs twice as long 6.2 / 4.6).  Here omega
// goes first: inverse transform, last radix-3 stage in registers, and its grid values STAY in registers (9 complex per item) while
//   F1 = omega x U    is formed, transformed forward through the same buffer and stored, then
//   B_f               is staged, transformed, and F2' = omega x B_f goes forward and is added to the running sum.
// Same arithmetic per element as X_FUSED_ADJ, 3 * HP transforms in the tile => tiles of twice as many points (128 / 64-byte runs).
// BONLY (X_FUSED_ADJ_B, a frozen-velocity context): nobody asks for dJ/dU, so the pass ends after F1's store — no prefetch of B_f, no
// running sum, no second staging / transform / accumulate.  What remains is the first half unchanged, expression by expression, so
// that dJ/dB0 comes out bit for bit as from the full pass.
// ---------------------------------------------------------------------------------------------------------
template <int L, int T, int NT, bool BONLY = false, bool WHOLE = false, class TW>
__device__ __forceinline__ void x_tile_adj_seq(const XSpec& sp, const double* __restrict__ gridU, const Geom& g, cplx* buf, const TW tw,
                                               const size_t i0, const int tid) {
    constexpr int HP = T / 2, NB = 3 * HP, S3 = L / 3;
    constexpr XLayout<L, NB, true> ix{};
    constexpr int NITEM = S3 * 3 * HP;                         // stored modes of one field group = items of the staging / split loops
    constexpr int SCNT = (NITEM + NT - 1) / NT;
    constexpr int ICNT = (HP * S3 + NT - 1) / NT;              // middle-section items (j, p) per thread
    // WHOLE (the two-wave shape) and the items divide evenly among the threads: every thread has all its items, no index needs a guard
    // either.  Not a nicety: an array that is written under a guard is merged with its previous contents, so omega's, U's and B_f's grid
    // values and the requested spectra become live ranges that span the kernel — with the guards the two-item form spills 36 registers at
    // an estimated peak of 175 live ones, without them none.  (The one-item form keeps its guards: the kernel it was.)
    constexpr bool ALLIT = WHOLE && ICNT * NT == HP * S3, ALLSP = WHOLE && SCNT * NT == NITEM;
    using S = Shape<L>;                                        // XSHEAD, XSTAIL, XSPRE, XSREQ, XSUEARLY: the SMO_X_SEQ_* knobs
    static_assert(last_radix<L, S::XSHEAD>() == 3, "G = 3N/2: the last Stockham stage is radix 3");
    const size_t plane = (size_t)g.G * g.Gzl;
    // WHOLE: the launch guarantees that T divides the plane (every tile is a whole one), so no line of it needs a guard
    auto line_ok = [&](int p) { return WHOLE || i0 + 2 * p < plane; };
    auto st_buf = [&](int b, int pos, cplx v) { buf[ix(b, pos)] = v; };
    static_assert(T <= 8, "a tile lies inside one z block of Ty");
    const XOrigin xo = x_origin(i0, g);
    auto spec_off = [&](int c, int kx, int p) -> size_t { return xo.base + c * xo.cs + kx * xo.ks + 2 * p; };

    // the first PRE (of SCNT) spectral items of B_f per thread are requested before the last forward stage of F1 (SMO_X_SEQ_PREFETCH)
    constexpr int PRE = BONLY ? 0 : (S::XSPRE < SCNT ? S::XSPRE : SCNT);
    cplx pre_in[PRE > 0 ? PRE : 1][2];
    auto request_in = [&](const cplx* src) {                   // the first PRE loads of stage_in, issued early
#pragma unroll
        for (int i = 0; i < PRE; ++i) {
            const int t = tid + i * NT, p = t % HP, r = t / HP, c = r % 3, kx = r / 3;
            pre_in[i][0] = mk(0, 0); pre_in[i][1] = mk(0, 0);
            if ((ALLSP || t < NITEM) && line_ok(p)) { const cplx* q = src + spec_off(c, kx, p); pre_in[i][0] = ld_cplx(q); pre_in[i][1] = ld_cplx(q + 1); }
        }
    };
    auto stage_in = [&](const cplx* src, auto requested, auto&& before_head) {           // spectra of one field group -> Hermitian-extended lines in the tile
#pragma unroll
        for (int i = 0; i < SCNT; ++i) {
            const int t = tid + i * NT;
            if (!ALLSP && t >= NITEM) break;
            const int p = t % HP, r = t / HP, c = r % 3, kx = r / 3;
            cplx X1 = mk(0, 0), X2 = mk(0, 0);
            if (decltype(requested)::value && i < PRE) { X1 = pre_in[i][0]; X2 = pre_in[i][1]; }
            else if (line_ok(p)) { const cplx* q = src + spec_off(c, kx, p); X1 = ld_cplx(q); X2 = ld_cplx(q + 1); }
            const int b = c * HP + p;
            if (kx == 0) buf[ix(b, 0)] = mk(X1.re, X2.re);
            else {
                buf[ix(b, kx)] = mk(X1.re - X2.im, X1.im + X2.re);
                buf[ix(b, L - kx)] = mk(X1.re + X2.im, X2.re - X1.im);
            }
        }
        before_head();
        __syncthreads();
        fft_inplace_head_r<S::XSHEAD, L, true, NB, NT, true, true>(buf, ix, tw, tid, [&](int b, int pos) -> cplx {
            return (pos >= L / 3 && pos <= L - L / 3) ? mk(0, 0) : buf[ix(b, pos)];
        });
    };
    auto read_win = [&](cplx (&W)[ICNT][3][3]) {                // [item][component][k]: inputs of the last inverse stage
#pragma unroll
        for (int i = 0; i < ICNT; ++i) {
            const int t = tid + i * NT, j = t / HP, p = t - j * HP;
            if ((ALLIT || t < HP * S3) && line_ok(p))
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    for (int k = 0; k < 3; ++k) W[i][c][k] = buf[ix(c * HP + p, j + S3 * k)];
        }
    };
    auto cross_first = [&](const cplx (&X)[3][3], const cplx (&Y)[3][3], int j, int p) {      // X x Y at the item's three points -> first forward stage
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            cplx v[3];
            for (int k = 0; k < 3; ++k)
                v[k] = mk(X[c1][k].re * Y[c2][k].re - X[c2][k].re * Y[c1][k].re, X[c1][k].im * Y[c2][k].im - X[c2][k].im * Y[c1][k].im);
            Butterfly<3, false>::run(v);
            const int b = c * HP + p;
            buf[ix(b, 3 * j)] = v[0];
            buf[ix(b, 3 * j + 1)] = twmul<false>(v[1], tw[j]);
            buf[ix(b, 3 * j + 2)] = twmul<false>(v[2], tw[2 * j]);
        }
    };
    cplx old_sum[BONLY ? 1 : SCNT][2];
    // the requests of a forward tail — B_f's spectra in the first half, the running sum in the second — are issued before its last stage, or
    // before the whole tail (SMO_X_SEQ_REQ_EARLY)
    auto forward_and_store = [&](cplx* dst, const bool acc) {
        auto requests = [&]() {
            if constexpr (!BONLY) {
                if (!acc && PRE > 0) request_in(sp.inB);
                if (acc) {
#pragma unroll
                    for (int i = 0; i < SCNT; ++i) {
                        const int t = tid + i * NT, p = t % HP, r = t / HP, c = r % 3, kx = r / 3;
                        if ((ALLSP || t < NITEM) && line_ok(p)) {
                            const cplx* q = dst + spec_off(c, kx, p);
                            old_sum[i][0] = q[0]; old_sum[i][1] = q[1];
                        }
                    }
                }
            }
        };
        if (S::XSREQ) requests();
        InplaceTail<L, L / 3, 3, false, NB, NT, true, true, S::XSTAIL>::run_ix(buf, ix, tid, tw, st_buf, [&]() { if (!S::XSREQ) requests(); });
        __syncthreads();
#pragma unroll
        for (int i = 0; i < SCNT; ++i) {
            const int t = tid + i * NT;
            if (!ALLSP && t >= NITEM) break;
            const int p = t % HP, r = t / HP, c = r % 3, kx = r / 3;
            if (!line_ok(p)) continue;
            const cplx Zk = buf[ix(c * HP + p, kx)];
            const cplx Zm = conj(buf[ix(c * HP + p, (kx == 0) ? 0 : L - kx)]);
            cplx* q = dst + spec_off(c, kx, p);
            cplx v0 = 0.5 * (Zk + Zm), v1 = mul_mi(0.5 * (Zk - Zm));
            if constexpr (!BONLY) { if (acc) { v0 = v0 + old_sum[i][0]; v1 = v1 + old_sum[i][1]; } }
            q[0] = v0;
            q[1] = v1;
        }
    };

    // ---- omega: spectrum -> grid, kept in registers -------------------------------------------------------------------------
    cplx Wom[ICNT][3][3], Wy[ICNT][3][3];
    // the velocity is requested before omega's inverse transform or after it (SMO_X_SEQ_U_EARLY)
    auto request_U = [&]() {
#pragma unroll
        for (int i = 0; i < ICNT; ++i) {
            const int t = tid + i * NT, j = t / HP, p = t - j * HP;
            if ((ALLIT || t < HP * S3) && line_ok(p))
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    for (int k = 0; k < 3; ++k) Wy[i][c][k] = ld_pair<NT_VELOCITY>(gridU + u_off(c, j + S3 * k, i0 + 2 * p, g));
        }
    };
    stage_in(sp.inA, std::false_type(), [&]() { if (S::XSUEARLY) request_U(); });
    read_win(Wom);
    if (!S::XSUEARLY) request_U();                      // requested before the barrier: in flight while the others read
    __syncthreads();
    // ---- F1 = omega x U -> forward -> out A --------------------------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < ICNT; ++i) {
        const int t = tid + i * NT, j = t / HP, p = t - j * HP;
        if ((!ALLIT && t >= HP * S3) || !line_ok(p)) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) Butterfly<3, true>::run(Wom[i][c]);
        cross_first(Wom[i], Wy[i], j, p);
    }
    __syncthreads();
    forward_and_store(sp.outA, false);
    if constexpr (!BONLY) {
        __syncthreads();
        // ---- B_f: spectrum -> grid; F2' = omega x B_f -> forward -> running sum (out B) -------------------------------------------
        stage_in(sp.inB, std::integral_constant<bool, (PRE > 0)>(), []() {});
        read_win(Wy);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ICNT; ++i) {
            const int t = tid + i * NT, j = t / HP, p = t - j * HP;
            if ((!ALLIT && t >= HP * S3) || !line_ok(p)) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) Butterfly<3, true>::run(Wy[i][c]);
            cross_first(Wom[i], Wy[i], j, p);
        }
        __syncthreads();
        forward_and_store(sp.outB, true);
    }
}

// One tile per workgroup.  PAIRED = P > 1: the tile is narrower than a 128-byte line of the spectra (T = 8/P complex), so the P
// tiles of a line are given to workgroups b, b+8, ..., which the dispatcher places on the same XCD at about the same time: the
// rest of every line is then served by that XCD's L2 instead of being fetched from HBM again (speed only, never correctness).
template <int L, int MODE, int T, int NT, int PAIRED = 0>         // PAIRED = tiles per 128-byte line of the spectra (0/1: no remapping)
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(MODE == X_FUSED_ADJ_SEQ ? Shape<L>::xs_waves(NT) : MODE == X_FUSED_ADJ_B ? Shape<L>::XBWAVES : Shape<L>::XWAVES))) void kd_x_pass(XSpec sp, const double* __restrict__ gridU, double* gridOut,
                                                const cplx* __restrict__ tw_g, Geom g) {
    constexpr bool FUSED = (MODE == X_FUSED_FWD || MODE == X_FUSED_ADJ || MODE == X_FUSED_ADJ_SEQ || MODE == X_FUSED_ADJ_B);
    constexpr int NB = ((MODE == X_FUSED_ADJ) ? 2 : 1) * 3 * (T / 2);
    __shared__ cplx buf[XLayout<L, NB, FUSED>::ELEMS];
    {   // batch member (Geom::mt / mg): the spectra, the grid field the mode reads, the grid vector it writes
        const size_t mt = blockIdx.y * g.mt;
        sp.inA += mt; sp.inB += mt; sp.outA += mt; sp.outB += mt;
        if constexpr (MODE == X_TO_GRID) gridOut += blockIdx.y * g.mg;
        else gridU += blockIdx.y * g.mg;
    }
    // G > 192: half twiddle table — with the full one (6 KB at G = 384) the tile fits only three times into a CU's LDS instead of four
    constexpr bool HALF = (L > 192);
    constexpr int NTW = HALF ? L / 2 : L;
    __shared__ cplx tw_s[NTW];
    const int tid = threadIdx.x;
    for (int i = tid; i < NTW; i += NT) tw_s[i] = tw_g[i];
    // a member whose horizon has not begun / is over (Geom::Nh): the fused passes of its step are not run — the adjoint pass in particular must
    // not go on adding omega x B_f to the running sum.  The grid <-> spectrum modes serve setup and output: every member, always.
    if constexpr (FUSED) { if (member_idle(g)) return; }
    // no barrier here for the fused tiles: they stage their spectra into the tile buffer first and put a barrier behind that loop before the
    // first butterfly reads a twiddle, so the table's loads and the spectra's are in flight together
    if (!FUSED) __syncthreads();
    size_t tile = blockIdx.x;
    if (PAIRED > 1 && blockIdx.x < (gridDim.x / (8 * PAIRED)) * (8 * PAIRED)) {
        const unsigned q = blockIdx.x / (8 * PAIRED), r = blockIdx.x % (8 * PAIRED);
        tile = (size_t)q * (8 * PAIRED) + PAIRED * (r % 8) + r / 8;
    }
    size_t i0 = tile * T;
    if constexpr (T <= 8) {
        if (g.tyl) {
            // z-block-major Ty: walk the tiles y-fastest inside a z block (the 8/T tiles of a 128-byte line first, then y, then the block):
            // consecutive workgroups then read consecutive lines of every kx block (a tile is independent of all others: any order is valid)
            constexpr unsigned PER = 8 / T;
            const size_t line = tile / PER, sub = tile - line * PER;
            const size_t zb = line / g.G, y = line - zb * g.G;
            i0 = y * g.Gzl + zb * 8 + sub * T;
        }
    }
    if constexpr (MODE == X_FUSED_ADJ_B) {
        if constexpr (HALF) x_tile_adj_seq<L, T, NT, true>(sp, gridU, g, buf, HalfTwiddles{tw_s, L / 2}, i0, tid);
        else x_tile_adj_seq<L, T, NT, true>(sp, gridU, g, buf, (const cplx*)tw_s, i0, tid);
    } else if constexpr (MODE == X_FUSED_ADJ_SEQ) {
        constexpr bool TWO = NT < Shape<L>::XITEMS;         // the two-wave shape: launched on whole tiles only
        if constexpr (HALF) x_tile_adj_seq<L, T, NT, false, TWO>(sp, gridU, g, buf, HalfTwiddles{tw_s, L / 2}, i0, tid);
        else x_tile_adj_seq<L, T, NT, false, TWO>(sp, gridU, g, buf, (const cplx*)tw_s, i0, tid);
    } else {
        if constexpr (HALF) x_tile<L, MODE, T, NT>(sp, gridU, gridOut, g, buf, HalfTwiddles{tw_s, L / 2}, i0, tid);
        else x_tile<L, MODE, T, NT>(sp, gridU, gridOut, g, buf, (const cplx*)tw_s, i0, tid);
    }
}

// ---------------------------------------------------------------------------------------------------------
// small per-mode kernels
// ---------------------------------------------------------------------------------------------------------
// compatibility condition: G = P(-2 B_N) / (dt alpha)  (Final)  |  / alpha (Integrated);  continuous: G = -2 B_N
__global__ void kd_terminal(const cplx* __restrict__ BN, cplx* __restrict__ Gh, cplx* __restrict__ nu, Geom g, int integrated, int continuous) {
    const size_t nmode = (size_t)g.al * g.m * g.m;
    BN += blockIdx.y * g.mc; Gh += blockIdx.y * g.mc;                               // batch member
    if (nu) nu += blockIdx.y * g.mc;                                                // (null: a frozen-velocity context has no nu^)
    const double Rm = g.Rmb ? g.Rmb[blockIdx.y] : g.Rm;                             // ... and its own Rm where the context has a table
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < nmode; e += (size_t)gridDim.x * blockDim.x) {
        const int iz = e % g.m, iy = (e / g.m) % g.m, ixl = e / ((size_t)g.m * g.m);
        const double k[3] = {(double)(g.ix0 + ixl), wavenumber(iy, g), wavenumber(iz, g)};
        const double k2 = k[0] * k[0] + k[1] * k[1] + k[2] * k[2];
        cplx r[3];
        for (int c = 0; c < 3; ++c) { cplx b = BN[c * nmode + e]; r[c] = mk(-2.0 * b.re, -2.0 * b.im); if (nu) nu[c * nmode + e] = mk(0, 0); }
        if (!continuous) {
            if (k2 == 0.0) { for (int c = 0; c < 3; ++c) r[c] = mk(0, 0); }
            else {
                const double alpha = 1.0 / g.dt + 0.5 * k2 / Rm, s = integrated ? alpha : g.dt * alpha, ik2 = 1.0 / k2;
                const cplx kr = mk((k[0] * r[0].re + k[1] * r[1].re + k[2] * r[2].re) * ik2, (k[0] * r[0].im + k[1] * r[1].im + k[2] * r[2].im) * ik2);
                for (int c = 0; c < 3; ++c) r[c] = mk((r[c].re - k[c] * kr.re) / s, (r[c].im - k[c] * kr.im) / s);
            }
        }
        for (int c = 0; c < 3; ++c) Gh[c * nmode + e] = r[c];
    }
}

// spectral energy  sum_k w |B^|^2  (w = 1 on the kx = 0 plane, 2 elsewhere) == grid mean of |B|^2 ; one partial per workgroup, one row of
// gridDim.x partials per batch member, `prow` doubles apart
__global__ __launch_bounds__(256) void kd_energy(const cplx* __restrict__ Bh, double* __restrict__ partial, Geom g, size_t prow) {
    __shared__ double red[4];
    const size_t nmode = (size_t)g.al * g.m * g.m, plane = (size_t)g.m * g.m;
    Bh += blockIdx.y * g.mc; partial += blockIdx.y * prow;
    double acc = 0.0;
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < nmode; e += (size_t)gridDim.x * 256) {
        const int ixl = e / plane;
        const double w = (g.ix0 + ixl == 0) ? 1.0 : 2.0;
        double s = 0.0;
        for (int c = 0; c < 3; ++c) { cplx b = Bh[c * nmode + e]; s += b.re * b.re + b.im * b.im; }
        acc += w * s;
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// batch member blockIdx.y: vectors of n doubles each, `n` apart; partials `prow` apart.  An odd n (odd G) puts every second member off a 16-byte
// boundary: those members read their pairs as two 8-byte loads (same pairs, same sums)
__global__ __launch_bounds__(256) void kd_dot(const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ partial, size_t n,
                                              size_t prow) {
    __shared__ double red[4];
    double acc = 0.0;
    x += blockIdx.y * n; y += blockIdx.y * n; partial += blockIdx.y * prow;
    const size_t n2 = n / 2;
    const double2* x2 = reinterpret_cast<const double2*>(x);
    const double2* y2 = reinterpret_cast<const double2*>(y);
    const bool a16 = ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(y)) & 15) == 0;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n2; i += (size_t)gridDim.x * 256) {
        double2 a, b;
        if (a16) { a = x2[i]; b = y2[i]; }
        else { a.x = x[2 * i]; a.y = x[2 * i + 1]; b.x = y[2 * i]; b.y = y[2 * i + 1]; }
        acc += a.x * b.x + a.y * b.y;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && (n & 1)) acc += x[n - 1] * y[n - 1];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// ---------------------------------------------------------------------------------------------------------
// the same passes with the transform length a run-time value: every even Npts without a tuned instantiation
// ---------------------------------------------------------------------------------------------------------
#include "kdyn_any.hpp"

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
constexpr int NPART = 1024;         // workgroups (= partial sums) of the reduction kernels

// Environment knobs of the KDYN context: this declaration is the list.  KDyn::init() reads them all, once, before anything else
// (SMO_SLAB_CHUNKS alone is read later, when a communicator attaches: comm_attach).
struct KDynEnv {
    bool any = env_is1("SMO_KD_ANY");                            // run-time-length kernels at a tuned size too (how the tests compare the two paths)
    int any_nt = env_int("SMO_KD_ANY_NT", 0);                    // ... their threads per workgroup: a multiple of 64 in 64..1024, anything else is ignored
    bool fuse_next = env_on("SMO_KD_FUSE_NEXT");                 // 0: the next step's inverse z pass as a kernel of its own (ablation)
    bool adj_seq = env_on("SMO_KD_ADJ_SEQ");                     // 0: adjoint x pass with both field groups in the tile at once (X_FUSED_ADJ)
    bool wt = env_on("SMO_KD_WT");                               // 0: plain stores on every hand-over stream (the build's write-through mask: SMO_KD_WT at the top; ablation, tests)
    int seq_items = env_int("SMO_KD_ADJ_SEQ_ITEMS", 0);          // 1: the one-item-per-thread shape of that pass where the build's default is the two-wave one (ablation, tests)
    int graph = env_int("SMO_KD_GRAPH", -1);                     // HIP graphs: -1 = grids up to SMO_KD_GRAPH_MAXG, 0 = never, 1 = always
    int graph_maxg = env_int("SMO_KD_GRAPH_MAXG", 36);
    int typad = env_int("SMO_KD_TYPAD", 8);                      // padding of a Ty plane / kx block, elements: a multiple of 8 (one 128-byte line)
    int tyl = env_int("SMO_KD_TYL", -1);                         // layout of Ty: 0 = planes, 1 = z-block major (ignored where it cannot apply), unset: by grid size
    int tyl_ming = env_int("SMO_KD_TYL_MING", 0);                // ... smallest grid that takes the z-block layout by default
    int ykx = env_int("SMO_KD_YKX", -1);                         // y pass, z-block-major Ty: 0 / 1 = workgroups z-fastest / kx-fastest, unset: per direction
    bool tystack = env_on("SMO_KD_TYSTACK");                     // 0: no grid-side stack of the forward states
    bool tycache = env_on("SMO_KD_TYCACHE");                     // 0: no Ty cache of the checkpoint window being replayed
    bool dense_tail = env_on("SMO_KD_DENSE_TAIL");               // 0: uniform checkpoint schedule
    bool dense_from_set = env_set("SMO_KD_DENSE_FROM");          // present at all: a dense tail with an explicit interval too (tests), starting at ...
    int dense_from = env_int("SMO_KD_DENSE_FROM", 0);            // ... this index (rounded down to a multiple of the interval)
    bool peer_chained = env_on("SMO_PEER_CHAINED");              // 0: full rendezvous protocol for the exchanges of the time loop
    bool force_exchange = env_is1("SMO_SLAB_FORCE_EXCHANGE");    // 1: one rank sends its transposes through the communicator (a self-exchange)
};

class KDyn : public Context {
public:
    explicit KDyn(const smo_config& c) { cfg = c; }

    // ---- state: geometry ----------------------------------------------------------------------------------------------------
    KDynEnv env;                             // filled at the top of init()
    Geom g{};
    size_t nmode = 0, tzb = 0, n_ex = 0, n_grid = 0, fld = 0;
    // tzb = 3*al*m*Gzr: one field group of Tz, per peer;  n_ex = 2*W*tzb: a whole exchange buffer (two field groups, all peers)
    // fld = 3*a*G*Gzr:  one field group of Ty (all kx, local z planes) = what the x pass reads
    // The rank's z slab can be cut into K equal chunks (SMO_KD_SET_CHUNKS): the grid-side phases then work chunk by chunk and every
    // chunk of an exchange buffer is contiguous, so the host layer can overlap the exchange of one chunk with the work on another.
    int K = 1;
    size_t tzc = 0, fldc = 0, ngc = 0;       // per chunk: tzb / K, 3*a*typ, n_grid / K
    static constexpr int TY_KMAX = 8;
    size_t ty_pad = 0;                       // SMO_KD_TYPAD, elements
    // run-time-length path (kdyn_any.hpp)
    bool any_size = false;
    int wt_mask = 0;                         // write-through streams of this context's launches (SMO_KD_WT)
    AnyPlan plan{};
    size_t any_lds = 65536;
    int any_nt = 512;                        // threads per workgroup of the any-size kernels (SMO_KD_ANY_NT)
    // Members with their own horizon (smo_set_horizons; Context::horizons, empty = none): d_hz is the device table the kernels read at
    // blockIdx.y (Geom::Nh; captured graphs hold its address, so new values go INTO it).  Member b runs N_b <= N = cfg.n_iters steps, right-aligned:
    // it idles through the first s_b = N - N_b steps of the launch sequence (its state is handed on unchanged) and runs its own last, so every
    // member's final state is snap(N) and member time i is state s_b + i.  act_now is the threshold of the step being enqueued (Geom::act):
    //   forward step n       takes the members with n >= s_b,   i.e. N_b >= N - n;
    //   adjoint iteration it takes the members with it < N_b,   i.e. N_b >= it + 1  (discrete sweep: it = N - 1 - idx, continuous: it = N - idx);
    // 0 outside the steps: every member takes part in setup, terminal condition and gradient output.
    int* d_hz = nullptr;
    int act_now = 0;

    // ---- state: buffers -----------------------------------------------------------------------------------------------------
    // Batched contexts: a slot holds every member's state, [slot][member][3][nmode] (snap(n) = the slot, member b at b * g.mc)
    cplx *d_stack = nullptr, *d_scratch = nullptr;
    cplx *d_ty = nullptr, *d_G = nullptr, *d_nu = nullptr, *d_tw = nullptr;
    cplx* d_acc = nullptr;                  // running sum of the adjoint's second product, the layout of Ty (nu_B / nu_C)
    // Ty stack (keep-all, enough HBM): the inverse y pass of B^_n writes to its own HBM slot instead of the work buffer; the adjoint
    // step then reads B_f from there: no z / y pass of the snapshot (2 of its 8 kernels) and, with slabs, one field group less to
    // exchange.
    cplx* d_tystack = nullptr;
    cplx* d_tycache = nullptr;              // checkpoint windows: Ty(B^_n) of the window being replayed, [ck][fld]
    cplx *zs = nullptr, *ys = nullptr;      // Tz exchange buffers: z-pass side / y-pass side (one and the same when world == 1)
    double *d_U = nullptr, *d_part = nullptr, *d_red = nullptr;
    double* d_Rm = nullptr;                 // smo_create_members: [batch] Rm values, written once here (captured graphs hold its address)
    double* d_tgrid = nullptr;              // smo_transform's grid vector
    std::vector<double> h_part;
    size_t n_part_rows = 1;

    // ---- state: schedule (ckpt_plan.hpp; walked on the CPU by tests/c/kdyn_plan_test.cpp) --------------------------------------
    // A state of the dense tail costs its adjoint step the z and y passes of the snapshot (no grid-side copy is kept for it), a recomputed
    // window a whole forward step per ck adjoint steps plus the grid-side form of its last state: ~0.58 against ~1.07 ms per adjoint step at 256^3.
    // Frozen velocity (smo_create_frozen_u): the context computes dJ/dB0 alone.  The G^ recursion reads U and the old G^ only, so
    // the adjoint x pass runs its omega x U half (X_FUSED_ADJ_B), nothing grid-side is kept (no Ty stack, no Ty cache, no running sum, no nu^),
    // and with the Final cost the sweep reads ONE forward state, B^_N: pingpong (keep_states = 0) then keeps no stack at all.
    ckpt::Schedule sched;
    int scratch_window = -1;                // the window the scratch slots hold
    int tycache_window = -1, tycache_count = 0;

    // ---- state: pipeline ----------------------------------------------------------------------------------------------------
    // zs_ready_*: the z-side buffer already holds the inverse z pass of snapshot n / of curl(G^) for adjoint index idx, left there by
    // the update kernel of the step before (NX_*); every other writer of the z-side buffer clears them.
    int zs_ready_fwd = -1, zs_ready_adj = -1;
    bool adj_cont = false;
    bool fuse_next = true;                   // SMO_KD_FUSE_NEXT, and never with the run-time-length kernels
    SlabComm comm;
    bool force_exchange = false;             // SMO_SLAB_FORCE_EXCHANGE on one rank
    hipStream_t cstream = nullptr;           // exchanges of the chunk pipeline (K > 1) run here, next to the kernels on `stream`
    hipEvent_t ev_main = nullptr;
    std::vector<hipEvent_t> ev_in, ev_ph, ev_out;
    // host time this rank spent ISSUING the last forward + adjoint solve: from the entry of the call to the point where everything is
    // enqueued, minus the time spent waiting for the other ranks in host rendezvous (smo_get key 4, milliseconds)
    double issue_ms_fwd = 0.0, issue_ms_adj = 0.0;

    // ---- state: graphs (see use_graph) --------------------------------------------------------------------------------------
    bool graph_broken = false;
    hipGraphExec_t gx_fwd = nullptr, gx_adj[2] = {nullptr, nullptr};
    struct Flags { int zf, za; bool cont; } fl_fwd{}, fl_adj[2]{};
    double *d_xin[2] = {nullptr, nullptr}, *d_gout[2] = {nullptr, nullptr};
    long long graph_replays = 0;

    // ---- state: timing classes (the indices are ABI to the benchmark: init_timing) ------------------------------------------
    int k_zi = -1, k_zic = -1, k_yi = -1, k_yf = -1, k_xf = -1, k_xa = -1, k_zfu = -1, k_zfa = -1, k_misc = -1, k_ex = -1, k_dot = -1, k_xb = -1;

    size_t nbatch() const { return (size_t)cfg.batch; }
    size_t slot_elems() const { return nbatch() * 3 * nmode; }
    cplx* snap(int n) {
        const ckpt::Slot s = sched.slot(n);
        return (s.scratch ? d_scratch : d_stack) + s.index * slot_elems();
    }
    // make state `idx` available (recompute its window from the preceding checkpoint if it is not resident)
    int ensure(int idx) {
        if (sched.resident(idx, scratch_window)) return SMO_OK;
        const int w = sched.window(idx), first = sched.first(w), last = sched.last(w);
        scratch_window = w;
        // the forward steps that rebuild the window pass through the grid-side form Ty(B^_n) of the states they start from: keep it
        // (one slot per step of the window), so that the adjoint steps of those states neither transform their snapshot again nor
        // send it — for ck = 2 that is every second adjoint step: two kernels and one exchanged field group less
        tycache_window = d_tycache ? w : -1;
        tycache_count = last - first;
        for (int n = first; n < last; ++n) SMO_TRY(step_fwd(n, d_tycache != nullptr));
        if (d_tycache && last < cfg.n_iters) {
            // ... and of the last state of the window: its inverse z pass is already in the exchange buffer (left by the update that
            // produced it), one y pass puts it beside the others — every adjoint step of the window then runs with one field group
            tycache_count += 1;
            SMO_TRY(fwd_A(last));
            for (int k = 0; k < K; ++k) { SMO_TRY(exchange(true, 1, k, stream)); SMO_TRY(y_pass(true, 0, 1, tyslot(last, k), k)); }
        }
        return SMO_OK;
    }
    Geom geom(int nfields, int k = 0) const { Geom q = g; q.blk = (size_t)nfields * tzc; q.cblk = (size_t)cfg.world * 2 * tzc; q.zg0 = k * g.Gzl; q.act = act_now; return q; }
    int first_state(size_t b) const { return horizons.empty() ? 0 : cfg.n_iters - horizons[b]; }      // s_b
    int check_horizons() override {
        if (cfg.world != 1 || force_exchange) {
            set_error("smo_set_horizons: a KDYN slab context (world = %d%s) runs one problem with one horizon; members with their own run on one GPU",
                      cfg.world, force_exchange ? ", self-exchange" : "");
            return SMO_ERR_UNSUPPORTED;
        }
        return SMO_OK;
    }
    int set_horizons(const int* n) override {
        have_forward = false;
        zs_ready_fwd = zs_ready_adj = -1; tycache_window = -1; scratch_window = -1; act_now = 0;
        const bool had = !horizons.empty();
        if (!n) {
            horizons.clear();
            g.Nh = nullptr;
            if (had) drop_graphs();                          // their nodes hold the table: back to the launches of a context without one
            return SMO_OK;
        }
        horizons.assign(n, n + cfg.batch);
        if (!d_hz) SMO_TRY(pool.alloc(&d_hz, nbatch()));
        SMO_HIP(hipMemcpyAsync(d_hz, horizons.data(), nbatch() * sizeof(int), hipMemcpyHostToDevice, stream));
        SMO_HIP(hipStreamSynchronize(stream));
        g.Nh = d_hz;
        if (!had) drop_graphs();                             // (new values in an existing table: the graphs stay, they read it when they run)
        return SMO_OK;
    }
    // Layout of Ty for the current chunk shape: z-block major (Geom::tyl, ty_off) when the local z planes come in whole blocks of 8 and the
    // tuned kernels run; SMO_KD_TYL = 0 / 1 forces the plane / z-block layout (1 is ignored where it cannot apply), SMO_KD_YKX = 0 keeps the
    // y pass's workgroups z-fastest.  fldc = elements of one field group of one chunk in whichever layout is larger.
    void pick_ty_layout() {
        const bool can = !any_size && g.Gzl % 8 == 0 && K <= TY_KMAX;
        const bool want = env.tyl >= 0 ? env.tyl == 1 : g.G >= env.tyl_ming;
        g.tyl = (can && want) ? 1 : 0;
        g.ykx = env.ykx >= 0 ? env.ykx : 1;      // (y_pass picks per direction)
        g.tyk = (size_t)g.G * 8 + (ty_pad ? ty_pad : 8);
        const size_t zb_elems = (size_t)(g.Gzl / 8) * g.tyk;          // per (component, kx): all its z blocks
        fldc = (size_t)3 * g.a * (g.tyl ? std::max(g.typ, zb_elems) : g.typ);
    }
    int set_chunks(int k) {
        const int Gzc = k > 0 ? g.Gzr / k : 0;
        // (one chunk of one slab may have any shape: odd G runs the run-time-length kernels, which pair its last line with zeros)
        if (k < 1 || g.Gzr % k != 0 || ((k > 1 || cfg.world > 1) && ((Gzc & 1) || ((size_t)g.G * Gzc) % 4 != 0))) {
            set_error("KDYN: %d chunks do not divide the %d local z planes into even parts with G*Gz %% 4 == 0", k, g.Gzr);
            return SMO_ERR_ARG;
        }
        K = k; g.Gzl = Gzc; tzc = tzb / K; ngc = n_grid / K;
        g.typ = (size_t)g.G * Gzc + (K <= TY_KMAX ? ty_pad : 0);
        pick_ty_layout();
        have_forward = false; zs_ready_fwd = zs_ready_adj = -1;
        return SMO_OK;
    }

    // ---- init: argument checks, geometry, schedule and allocations, timing classes ------------------------------------------
    int init() override {
        env = KDynEnv();
        SMO_TRY(check_args());
        SMO_TRY(init_geometry());
        SMO_TRY(base_init());
        SMO_TRY(init_any_lds());
        SMO_TRY(init_buffers());
        init_timing();
        return SMO_OK;
    }
    int check_args() {
        const int N = cfg.npts, W = cfg.world;
        // batch = B > 1: B independent problems of the same size and parameters on ONE GPU, member = blockIdx.y of every launch (Geom::mc ...)
        if (cfg.batch < 1 || (cfg.batch > 1 && W != 1)) { set_error("KDYN: batch %d with %d slabs (a batch runs on one GPU: world = 1)", cfg.batch, W); return SMO_ERR_ARG; }
        if (!member_params.empty() && (W != 1 || member_params.size() != (size_t)cfg.batch)) {
            set_error("KDYN: one Rm per member needs one GPU (world = 1) and %d values (got world = %d, %zu values)", cfg.batch, W, member_params.size());
            return SMO_ERR_ARG;
        }
        if (frozen_u && W != 1) { set_error("KDYN: a frozen-velocity context runs on one GPU (world = 1, got %d)", W); return SMO_ERR_UNSUPPORTED; }
        if (!keep_states && (!frozen_u || cfg.cost != SMO_COST_FINAL)) {
            set_error("KDYN: keep_states = 0 needs a frozen velocity and the Final cost (the Integrated adjoint reads every forward state B^_n in its z update)");
            return SMO_ERR_ARG;
        }
        if (cfg.batch > 65535) { set_error("KDYN: batch %d (at most 65535: the members are the second grid dimension)", cfg.batch); return SMO_ERR_UNSUPPORTED; }
        if (cfg.batch > 1 && env.force_exchange) {
            set_error("KDYN: SMO_SLAB_FORCE_EXCHANGE=1 with batch %d (the self-exchange is a single-problem test path)", cfg.batch);
            return SMO_ERR_UNSUPPORTED;
        }
        if (N < 6 || (N & 1)) { set_error("KDYN: npts must be even and >= 6 (got %d)", N); return SMO_ERR_UNSUPPORTED; }
        if ((N / 2) % W != 0 || (3 * N / 2) % W != 0 || (W > 1 && ((3 * N / 2 / W) * (3 * N / 2)) % 4 != 0)) {
            set_error("KDYN: %d slabs do not divide a=%d kx modes and G=%d grid planes", W, N / 2, 3 * N / 2);
            return SMO_ERR_UNSUPPORTED;
        }
        if (env.typad % 8 != 0) { set_error("KDYN: SMO_KD_TYPAD must be a multiple of 8 elements (one 128-byte line)"); return SMO_ERR_ARG; }
        return SMO_OK;
    }
    int init_geometry() {
        const int N = cfg.npts, W = cfg.world;
        fuse_next = env.fuse_next;
        ty_pad = (size_t)env.typad;
        force_exchange = W == 1 && env.force_exchange;
        // Tuned kernels: the transform lengths G = 3N/2 with factors 2, 3, 5 and 7 instantiated below (with_L, from the list of
        // kdyn_plan.hpp).  Every other even Npts — the reference, through FFTW, takes any (FWD_Solve_KDyn.py:362-450, :1029) — runs the
        // run-time-length kernels of kdyn_any.hpp (SMO_KD_ANY=1 forces them at a tuned size too: how the tests compare the two paths).
        any_size = env.any || !kdplan::is_tuned(3 * N / 2);      // (a tuned G is even: G * G % 4 == 0)
        wt_mask = 0;                                             // write-through streams in force: Shape<G>::WT unless SMO_KD_WT=0 (smo_get key 7)
        if (!any_size && env.wt) {
            switch (3 * N / 2) {
#define SMO_KD_CASE(L) case L: wt_mask = Shape<L>::WT; break;
                SMO_KD_TUNED_G(SMO_KD_CASE)
#undef SMO_KD_CASE
            }
        }
        g.a = N / 2; g.al = g.a / W; g.ix0 = cfg.rank * g.al; g.m = N - 1; g.kmax = (N - 1) / 2; g.G = 3 * N / 2; g.Gzl = g.Gzr = g.G / W; g.W = W; g.zg0 = 0;
        g.Rm = cfg.param; g.dt = cfg.dt;
        nmode = (size_t)g.al * g.m * g.m;
        tzb = (size_t)3 * g.al * g.m * g.Gzl;
        n_ex = 2 * tzb * W;                              // two field groups (adjoint) x peers
        if (any_size) {
            fuse_next = false;                               // the run-time-length update kernel has no fused next pass
            plan = any_plan(3 * N / 2);
            if (env.any_nt >= 64 && env.any_nt <= 1024 && env.any_nt % 64 == 0) any_nt = env.any_nt;
        }
        // One 128-byte line of padding per (component, kx) plane of Ty.  The x pass gathers 3a runs per tile, one per plane; with the
        // natural stride 16*G*Gzl (a multiple of 64 KB at every supported size) they all fall on the same HBM channel: measured
        // 240 -> 205 us for the fused adjoint x pass at 128^3.  SMO_KD_TYPAD (elements, a multiple of 8) overrides it for tuning.
        g.typ = (size_t)g.G * g.Gzl + ty_pad;
        // one field group of Ty, all chunks: the planes with their padding, or the z blocks with theirs (G/8... Gzr/8 blocks of 8 G + pad per kx)
        fld = (size_t)3 * g.a * ((size_t)g.G * g.Gzl + std::max((size_t)TY_KMAX * ty_pad, (size_t)(g.Gzl / 8 + 1) * std::max<size_t>(ty_pad, 8)));
        n_grid = (size_t)3 * g.G * g.G * g.Gzl;          // local slab of a grid vector: [3][G][G][Gzl]
        g.mc = 3 * nmode; g.mz = n_ex; g.mt = fld; g.mg = n_grid;      // member strides (batch): one member's copy of each buffer kind
        g.blk = tzb;
        tzc = tzb; ngc = n_grid;
        pick_ty_layout();
        n_comp = 2;
        vec_len = n_grid;
        snapshot_doubles = 2 * 3 * nmode;
        return SMO_OK;
    }
    // run-time-length kernels: LDS of one workgroup is 64 KB unless the narrowest tile of the adjoint x pass (3 buffers x 3 transforms + the
    // twiddle table) needs more
    int init_any_lds() {
        if (!any_size || (size_t)160 * plan.L <= any_lds) return SMO_OK;
        int dev = 0, maxb = 0;
        SMO_HIP(hipGetDevice(&dev));
        SMO_HIP(hipDeviceGetAttribute(&maxb, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
        if ((size_t)160 * plan.L > (size_t)maxb) { set_error("KDYN: G = %d needs %zu bytes of LDS per workgroup (device: %d)", plan.L, (size_t)160 * plan.L, maxb); return SMO_ERR_UNSUPPORTED; }
        any_lds = (size_t)maxb;
        SMO_HIP(hipFuncSetAttribute((const void*)kda_z_inverse, hipFuncAttributeMaxDynamicSharedMemorySize, maxb));
        SMO_HIP(hipFuncSetAttribute((const void*)kda_z_forward, hipFuncAttributeMaxDynamicSharedMemorySize, maxb));
        SMO_HIP(hipFuncSetAttribute((const void*)kda_y_pass, hipFuncAttributeMaxDynamicSharedMemorySize, maxb));
        SMO_HIP(hipFuncSetAttribute((const void*)kda_x_pass, hipFuncAttributeMaxDynamicSharedMemorySize, maxb));
        return SMO_OK;
    }
    int free_hbm(size_t* free_b) { size_t total_b = 0; SMO_HIP(hipMemGetInfo(free_b, &total_b)); return SMO_OK; }
    // The schedule and every allocation, in the order that decides what each hipMemGetInfo sees; the decisions themselves are kdyn_plan.hpp's.
    int init_buffers() {
        const int N = cfg.n_iters, W = cfg.world;
        const kdplan::KdSizes sz{nmode, n_ex, fld, n_grid, nbatch(), sizeof(cplx)};
        size_t free_b = 0;
        sched.N = N;
        sched.pingpong = frozen_u && !keep_states;
        sched.ck = sched.pingpong ? 1 : cfg.ckpt;            // (no stack: smo_config.ckpt is not consulted)
        if (sched.ck < 0) { set_error("KDYN: ckpt=%d", sched.ck); return SMO_ERR_ARG; }
        if (sched.ck == 0) {                                 // first interval that fits the free HBM
            SMO_TRY(free_hbm(&free_b));
            sched.ck = kdplan::pick_interval(N, sz, free_b);
        }
        const int ck = sched.ck = kdplan::clamp_interval(sched.ck, N);
        SMO_TRY(pool.upload(&d_tw, twiddles(g.G), stream));
        if (!member_params.empty()) {                        // members with their own Rm: the table the kernels read at blockIdx.y (Geom::Rmb)
            SMO_TRY(pool.upload(&d_Rm, member_params, stream));
            g.Rmb = d_Rm;
        }
        // a context with checkpoint windows on ONE GPU allocates its stack last, sized with a dense tail from what is then free (below)
        // (batch > 1: uniform windows only — no dense tail, no y-side stack; neither changes a bit of the results)
        const bool tail_ok = kdplan::tail_ok(ck, W, cfg.batch, cfg.ckpt, env.dense_from_set, env.force_exchange);
        if (!tail_ok) SMO_TRY(pool.alloc(&d_stack, sched.stack_slots() * slot_elems()));
        if (ck > 1) SMO_TRY(pool.alloc(&d_scratch, sched.scratch_slots() * slot_elems()));
        if (!frozen_u) {                                     // Ty stack (SMO_KD_TYSTACK=0 disables)
            SMO_TRY(free_hbm(&free_b));
            if (kdplan::ty_stack_fits(N, ck, sz, env.tystack, free_b)) SMO_TRY(pool.alloc(&d_tystack, (size_t)N * fld));
        }
        if (ck > 1 && !frozen_u) {                           // Ty cache of the window being replayed (SMO_KD_TYCACHE=0 disables)
            SMO_TRY(free_hbm(&free_b));
            if (kdplan::ty_cache_fits(ck, sz, env.tycache, free_b)) SMO_TRY(pool.alloc(&d_tycache, (size_t)ck * fld * nbatch()));
        }
        // per-member work buffers: member b's copy Geom::m* elements after member 0's (Ty: [field group][member][fld], the others [member][...])
        // (a frozen-velocity context: one field group of Ty, no running sum, no nu^)
        SMO_TRY(pool.alloc(&d_ty, (frozen_u ? 1 : 2) * fld * nbatch()));
        if (!frozen_u) SMO_TRY(pool.alloc(&d_acc, fld * nbatch()));
        // exchange buffers: one and the same on a single GPU; with slabs the z side and the y side are apart (a host layer that does
        // the transposes itself may still point the context at its own pair: SMO_KD_SET_BUFFERS).  SMO_SLAB_FORCE_EXCHANGE=1 keeps them
        // apart on ONE rank too, so that a one-GPU box sends every transpose through the real communicator (a self-exchange).
        SMO_TRY(pool.alloc(&zs, n_ex * nbatch()));
        if (W == 1 && !force_exchange) ys = zs;
        else SMO_TRY(pool.alloc(&ys, n_ex));
        SMO_TRY(pool.alloc(&d_red, 8));
        SMO_TRY(pool.alloc(&d_G, 3 * nmode * nbatch()));
        if (!frozen_u) SMO_TRY(pool.alloc(&d_nu, 3 * nmode * nbatch()));
        SMO_TRY(pool.alloc(&d_U, n_grid * nbatch()));
        // partial sums: [member][row][NPART] (row n = <B_n,B_n> of the integrated cost; row 0 also serves the inner product)
        n_part_rows = (cfg.cost == SMO_COST_INTEGRATED) ? (size_t)cfg.n_iters + 1 : 1;
        SMO_TRY(pool.alloc(&d_part, nbatch() * n_part_rows * NPART));
        h_part.resize(nbatch() * n_part_rows * NPART);
        if (tail_ok) {
            // dense tail: as many extra snapshots as the free HBM holds beyond the uniform stack.  SMO_KD_DENSE_FROM = n forces the first dense
            // index (tests), SMO_KD_DENSE_TAIL=0 keeps the uniform schedule.
            SMO_TRY(free_hbm(&free_b));
            sched.dense_from = kdplan::pick_dense_from(N, ck, kdplan::dense_fit(sz, free_b), env.dense_tail, env.dense_from_set, env.dense_from);
            SMO_TRY(pool.alloc(&d_stack, sched.stack_slots() * slot_elems()));
        }
        stack_bytes = (sched.stack_slots() + sched.scratch_slots()) * sz.slot_bytes() + (d_tystack ? (size_t)N * fld * sizeof(cplx) : 0);
        return SMO_OK;
    }
    void init_timing() {
        // algorithmic bytes per launch (every axis pass reads + writes its field; S0..S3 per component, per slab)
        // (a batched launch moves every member's share: x B)
        const double nb = (double)cfg.batch;
        const double S0 = nb * 16.0 * nmode, S1 = nb * 16.0 * g.al * g.m * (double)g.G, S2 = nb * 16.0 * g.a * (double)g.G * g.Gzl,
                     S3 = nb * 8.0 * (double)g.G * g.G * g.Gzl;
        // second figure = compulsory HBM bytes of the kernel as fused (every input read once, every output written once): the
        // denominator of the roofline fraction (the algorithmic count above it prices passes the fusion removed)
        k_zi = timing.add_class("kd_z_inverse", 3 * (S0 + S1));
        k_zic = timing.add_class("kd_z_inverse<curl>", 3 * (S0 + S1));
        k_yi = timing.add_class("kd_y_pass<inv>", 3 * (S1 + S2));
        k_yf = timing.add_class("kd_y_pass<fwd>", 3 * (S1 + S2));
        k_xf = timing.add_class("kd_x_pass<fused_fwd>", 3 * (2 * (S2 + S3) + 3 * S3),            // 3 c2r + 3 r2c passes + pointwise (read B,U write EMF)
                                6 * S2 + 3 * S3);                                             // fused: read B (Ty), U; write the EMF's spectrum
        k_xa = timing.add_class("kd_x_pass<fused_adj>", 3 * (4 * (S2 + S3) + 5 * S3),            // 6 c2r + 6 r2c + pointwise (read w,U,B_f write F1,F2)
                                15 * S2 + 3 * S3);                                            // fused: read w, B_f, U, the running sum; write F1, the sum
        const double nxt = fuse_next ? 3 * (S0 + S1) : 0.0;                                     // + the next step's inverse z pass, run on the same tile
        const double nxt_hbm = fuse_next ? 3 * S1 : 0.0;                                        // ... which only adds the write of Tz
        k_zfu = timing.add_class("kd_z_forward<fwd_update>", 3 * (S1 + S0) + 12 * S0 + nxt,    // 3 z passes + step (read B,N; write B, snapshot)
                                 3 * S1 + 6 * S0 + nxt_hbm);                                   // fused: read Tz, B_n; write B_{n+1} (the stack IS the state)
        k_zfa = timing.add_class("kd_z_forward<adj_update>", 3 * (S1 + S0) + 12 * S0 + nxt,    // F1 only: F2 is summed on the grid side (nu_B / nu_C)
                                 3 * S1 + 6 * S0 + (cfg.cost == SMO_COST_INTEGRATED ? 3 * S0 : 0.0) + nxt_hbm);
        k_misc = timing.add_class("kd_misc(setup/terminal/energy/grid io)", 0);
        // slab transposes: HIP events around every grouped send/recv on the stream it is issued on (one field group of one rank, all
        // peers, as the byte figure; an adjoint step without kept grid states sends two groups in one call)
        k_ex = timing.add_class("slab_exchange(all-to-all)", nb * 16.0 * tzb * cfg.world, 0.0);
        // Inner_Prod_3 (FWD_Solve_KDyn.py:173-181; SURVEY.md 8d: "2 x (vector bytes)" per call — 340 MB at 128^3, 2.72 GB at 256^3)
        k_dot = timing.add_class("kd_dot(inner product)", nb * 2.0 * 8.0 * (double)n_grid);
        // adjoint x pass of a frozen-velocity context (last, so that the indices above stay what they were): the forward pass's figures
        k_xb = timing.add_class("kd_x_pass<fused_adj_b>", 3 * (2 * (S2 + S3) + 3 * S3),          // 3 c2r + 3 r2c passes + pointwise (read w,U write F1)
                                6 * S2 + 3 * S3);                                             // fused: read w (Ty), U; write F1's spectrum
    }

    // ---- launch helpers -----------------------------------------------------------------------------------------
    template <class F> int with_L(F f) {
#ifdef SMO_KD_FEW_SIZES              // experimental builds (tools/kernel_resources.sh -DSMO_KD_FEW_SIZES): the two bench grids only, a tenth of the compile time
        switch (g.G) {
            case 192: return f(std::integral_constant<int, 192>());
            case 384: return f(std::integral_constant<int, 384>());
        }
        set_error("KDYN: grid %d not in this experimental build", g.G);
        return SMO_ERR_UNSUPPORTED;
#else
        switch (g.G) {
#define SMO_KD_CASE(L) case L: return f(std::integral_constant<int, L>());
            SMO_KD_TUNED_G(SMO_KD_CASE)
#undef SMO_KD_CASE
        }
        set_error("KDYN: unsupported grid %d", g.G);
        return SMO_ERR_UNSUPPORTED;
#endif
    }
    // run-time-length path (kdyn_any.hpp): largest tile of `unit` bytes per transform-row multiple that fits the LDS limit
    int any_tile(size_t bytes_per_unit, std::initializer_list<int> cands) const {
        for (int c : cands) if (((size_t)c * bytes_per_unit + 16) * plan.L <= any_lds) return c;      // + the twiddle table
        return *(cands.end() - 1);
    }

    int need_buffers() {
        if (!zs || !ys) { set_error("KDYN: slab exchange buffers not set (SMO_KD_SET_BUFFERS)"); return SMO_ERR_STATE; }
        return SMO_OK;
    }
    // workgroups of a launch, one timer per launch (the tuned kernels carry their own timestamps: SMO_LAUNCH_T)
    dim3 z_grid(int nbt) const { return dim3((g.al * g.m + nbt - 1) / nbt, cfg.batch); }             // z passes: nbt (kx, ky) columns each
    dim3 y_grid(int zt) const { return dim3(3 * g.a * ((g.Gzl + zt - 1) / zt), cfg.batch); }         // y pass: zt planes of one (component, kx)
    // coefficients -> field group `f` (of `nf`) of the z-side exchange buffer
    int z_inverse(int mode, const cplx* in, int f, int nf) {
        const Geom g = geom(nf);
        zs_ready_fwd = zs_ready_adj = -1;
        cplx* out = zs + (size_t)f * tzc;
        ScopedTimer t(timing, mode == ZI_CURL ? k_zic : (mode == ZI_PLAIN ? k_zi : k_misc), stream, !any_size);
        if (any_size) {
            const int NBT = any_tile(96, {2, 1});
            SMO_LAUNCH(kda_z_inverse, z_grid(NBT), dim3(any_nt), ((size_t)96 * NBT + 16) * plan.L, stream, in, out, (const cplx*)d_tw, g, plan, mode, NBT);
            return SMO_OK;
        }
        return with_L([&](auto l) {
            constexpr int L = decltype(l)::value;
            using S = Shape<L>;
            const dim3 grid = z_grid(S::ZNBT);
            if (mode == ZI_PLAIN) SMO_LAUNCH_T(t, (kd_z_inverse<L, ZI_PLAIN, S::ZNBT, S::ZNT>), grid, dim3(S::ZNT), 0, stream, in, out, d_tw, g);
            else if (mode == ZI_CURL) SMO_LAUNCH_T(t, (kd_z_inverse<L, ZI_CURL, S::ZNBT, S::ZNT>), grid, dim3(S::ZNT), 0, stream, in, out, d_tw, g);
            else SMO_LAUNCH_T(t, (kd_z_inverse<L, ZI_SCALE, S::ZNBT, S::ZNT>), grid, dim3(S::ZNT), 0, stream, in, out, d_tw, g);
            return SMO_OK;
        });
    }
    // y pass between field group `f` (of `nf`) of chunk `k` of the y-side exchange buffer and (that chunk of) one field group of Ty at `ty`
    int y_pass(bool inv, int f, int nf, cplx* ty, int k = 0) {
        Geom q = geom(nf, k);
        // z-block-major Ty: the inverse pass (reads Tz, WRITES Ty) takes its workgroups kx-fastest — adjacent blocks of Ty are written together
        // (256^3: 315 -> 289 us) —, the forward pass (reads Ty, writes Tz) z-fastest (265 vs 271 us kx-fastest); SMO_KD_YKX = 0 / 1 forces one order
        q.ykx = env.ykx >= 0 ? env.ykx : (inv ? 1 : 0);
        if (!inv && ys == zs) zs_ready_fwd = zs_ready_adj = -1;      // one GPU: the y pass writes the buffer the z pass reads
        cplx* ex = ys + (size_t)k * q.cblk + (size_t)f * tzc;
        ScopedTimer t(timing, inv ? k_yi : k_yf, stream, !any_size);
        if (any_size) {
            const int ZT = any_tile(32, {8, 4, 2, 1});
            SMO_LAUNCH(kda_y_pass, y_grid(ZT), dim3(any_nt), ((size_t)32 * ZT + 16) * plan.L, stream, inv ? (const cplx*)ex : (const cplx*)ty, inv ? ty : ex,
                               (const cplx*)d_tw, q, plan, inv ? 1 : 0, ZT);
            return SMO_OK;
        }
        return with_L([&](auto l) {
            constexpr int L = decltype(l)::value;
            using S = Shape<L>;
            auto launch = [&](auto zt) {
                constexpr int ZT = decltype(zt)::value;
                // (write-through streams, here and below: the kernel with the policy bits exists only where Shape<L>::WT has them)
                if constexpr (S::wt(WT_TY)) { if (inv && env.wt) { SMO_LAUNCH_T(t, (kd_y_pass<L, true, ZT, S::YNT, true>), y_grid(ZT), dim3(S::YNT), 0, stream, (const cplx*)ex, ty, d_tw, q); return; } }
                if constexpr (S::wt(WT_TZ)) { if (!inv && env.wt) { SMO_LAUNCH_T(t, (kd_y_pass<L, false, ZT, S::YNT, true>), y_grid(ZT), dim3(S::YNT), 0, stream, (const cplx*)ty, ex, d_tw, q); return; } }
                if (inv) SMO_LAUNCH_T(t, (kd_y_pass<L, true, ZT, S::YNT>), y_grid(ZT), dim3(S::YNT), 0, stream, (const cplx*)ex, ty, d_tw, q);
                else SMO_LAUNCH_T(t, (kd_y_pass<L, false, ZT, S::YNT>), y_grid(ZT), dim3(S::YNT), 0, stream, (const cplx*)ty, ex, d_tw, q);
            };
            // thin slabs: halve the z tile when that avoids a mostly empty last tile (e.g. 128^3 on 8 GPUs: 24 local planes)
            if (g.Gzl % S::YZT != 0 && g.Gzl % (S::YZT / 2) == 0) launch(std::integral_constant<int, S::YZT / 2>());
            else launch(std::integral_constant<int, S::YZT>());
            return SMO_OK;
        });
    }
    // chunk `k` of the grid stage.  vec_in / vec_out: caller-layout grid vectors (X_FROM_GRID / X_TO_GRID); vec_out == nullptr with
    // X_TO_GRID writes the internal (tile-major) U field.  inA / inB: read the spectra of field group A / B from elsewhere (the Ty stack).
    int x_pass(int mode, int k, const double* vec_in, double* vec_out, const cplx* inA = nullptr, const cplx* inB = nullptr) {
        const size_t plane = (size_t)g.G * g.Gzl;
        Geom q = geom(1, k);
        const bool to_U = (mode == X_TO_GRID && vec_out == nullptr);
        q.utile = to_U ? 1 : 0;
        double* Uk = d_U + (size_t)k * ngc;
        const double* grid_in = (mode == X_FROM_GRID) ? vec_in : Uk;
        double* grid_out = to_U ? Uk : vec_out;
        cplx *tA = tyw(0, k), *tB = frozen_u ? tA : tyw(1, k);         // (frozen velocity: Ty has one field group, no mode of it touches group B)
        const XSpec sp{inA ? inA : tA, inB ? inB : tB, tA, mode == X_FUSED_ADJ ? d_acc + (size_t)k * fldc : tB};
        auto tiles = [&](int T) { return dim3((unsigned)((plane + T - 1) / T), cfg.batch); };
        const int kc = mode == X_FUSED_FWD ? k_xf : (mode == X_FUSED_ADJ ? k_xa : (mode == X_FUSED_ADJ_B ? k_xb : k_misc));
        ScopedTimer t(timing, kc, stream, !any_size);
        if (any_size) {
            // the internal U field stays in the flat grid layout [3][G][G][Gzr] (all chunks in one array: Geom::zg0 places the chunk)
            q.utile = 0;
            const int nbuf = mode == X_FUSED_ADJ ? 3 : 2, HP = any_tile((size_t)48 * nbuf, {4, 2, 1});
            SMO_LAUNCH(kda_x_pass, tiles(2 * HP), dim3(any_nt), ((size_t)48 * nbuf * HP + 16) * plan.L, stream, sp, mode == X_FROM_GRID ? vec_in : (const double*)d_U,
                               to_U ? d_U : vec_out, (const cplx*)d_tw, q, plan, mode, HP);
            return SMO_OK;
        }
        return with_L([&](auto l) {
            constexpr int L = decltype(l)::value;
            using S = Shape<L>;
            switch (mode) {
                case X_TO_GRID: SMO_LAUNCH_T(t, (kd_x_pass<L, X_TO_GRID, S::XTG, S::XGNT>), tiles(S::XTG), dim3(S::XGNT), 0, stream, sp, grid_in, grid_out, d_tw, q); break;
                case X_FROM_GRID: SMO_LAUNCH_T(t, (kd_x_pass<L, X_FROM_GRID, S::XTG, S::XGNT>), tiles(S::XTG), dim3(S::XGNT), 0, stream, sp, grid_in, grid_out, d_tw, q); break;
                case X_FUSED_FWD: SMO_LAUNCH_T(t, (kd_x_pass<L, X_FUSED_FWD, S::XT, S::XNT, 8 / S::XT>), tiles(S::XT), dim3(S::XNT), 0, stream, sp, grid_in, grid_out, d_tw, q); break;
                case X_FUSED_ADJ_B: SMO_LAUNCH_T(t, (kd_x_pass<L, X_FUSED_ADJ_B, S::XBT, S::XBNT, 8 / S::XBT>), tiles(S::XBT), dim3(S::XBNT), 0, stream, sp, grid_in, grid_out, d_tw, q); break;
                default:
                    // adjoint: the field groups one after the other through the tile buffer (tiles as wide as the forward pass's), unless
                    // SMO_KD_ADJ_SEQ=0 asks for both at once in half-width tiles (round 1's kernel, kept for comparison)
                    // ... in the two-wave shape where the length has it (Shape<L>::XS2): one member, the whole grid in one launch — batched
                    // contexts, slabs and chunks keep the one-item shape, and SMO_KD_ADJ_SEQ_ITEMS=1 asks for it (how the tests compare the two)
                    if constexpr (S::XS2) {
                        if (env.adj_seq && env.seq_items != 1 && cfg.batch == 1 && q.Gzl == q.G && plane % S::XTS == 0) {
                            SMO_LAUNCH_T(t, (kd_x_pass<L, X_FUSED_ADJ_SEQ, S::XTS, S::XSNT2, 8 / S::XTS>), tiles(S::XTS), dim3(S::XSNT2), 0, stream, sp, grid_in, grid_out, d_tw, q);
                            break;
                        }
                    }
                    if (env.adj_seq) SMO_LAUNCH_T(t, (kd_x_pass<L, X_FUSED_ADJ_SEQ, S::XTS, S::XSNT, 8 / S::XTS>), tiles(S::XTS), dim3(S::XSNT), 0, stream, sp, grid_in, grid_out, d_tw, q);
                    else SMO_LAUNCH_T(t, (kd_x_pass<L, X_FUSED_ADJ, S::XTA, S::XANT, 8 / S::XTA>), tiles(S::XTA), dim3(S::XANT), 0, stream, sp, grid_in, grid_out, d_tw, q);
                    break;
            }
            return SMO_OK;
        });
    }
    // z-side exchange buffer (one field group) -> coefficients / time-step update [-> z-side buffer again: inverse z pass of the new
    // state, see NX_*]
    int z_forward(int mode, cplx* out0, const cplx* state0, const cplx* snp, int next = NX_NONE) {
        const Geom g = geom(1);
        const double scale = 1.0 / ((double)g.G * g.G * g.G);
        const int integ = cfg.cost == SMO_COST_INTEGRATED;
        ScopedTimer t(timing, mode == ZF_FWD_UPDATE ? k_zfu : (mode == ZF_ADJ_UPDATE ? k_zfa : k_misc), stream, !any_size);
        if (any_size) {
            const int NBT = any_tile(96, {2, 1});
            SMO_LAUNCH(kda_z_forward, z_grid(NBT), dim3(any_nt), ((size_t)96 * NBT + 16) * plan.L, stream, (const cplx*)zs, out0, state0, snp, (const cplx*)d_tw, g, plan,
                               mode, NBT, scale, integ);
            return SMO_OK;
        }
        return with_L([&](auto l) {
            constexpr int L = decltype(l)::value;
            using S = Shape<L>;
            const dim3 grid = z_grid(S::ZNBT), block(S::ZNT);
#define SMO_ZF(MODE_, NEXT_, WT_) SMO_LAUNCH_T(t, (kd_z_forward<L, MODE_, NEXT_, S::ZNBT, S::ZNT, WT_>), grid, block, 0, stream, (const cplx*)zs, out0, state0, snp, d_tw, g, scale, integ, zs)
            constexpr int WZ = S::WT & (WT_STATE | WT_NEXT), WZ0 = S::WT & WT_STATE;       // write-through streams of the update kernels with / without a NEXT tail
            if constexpr (WZ != 0) {
                if (env.wt && mode == ZF_FWD_UPDATE && next == NX_PLAIN) { SMO_ZF(ZF_FWD_UPDATE, NX_PLAIN, WZ); return SMO_OK; }
                if (env.wt && mode == ZF_ADJ_UPDATE && next == NX_CURL) { SMO_ZF(ZF_ADJ_UPDATE, NX_CURL, WZ); return SMO_OK; }
            }
            if constexpr (WZ0 != 0) {
                if (env.wt && mode == ZF_FWD_UPDATE && next != NX_PLAIN) { SMO_ZF(ZF_FWD_UPDATE, NX_NONE, WZ0); return SMO_OK; }
                if (env.wt && mode == ZF_ADJ_UPDATE && next != NX_CURL) { SMO_ZF(ZF_ADJ_UPDATE, NX_NONE, WZ0); return SMO_OK; }
            }
            if (mode == ZF_PLAIN) SMO_ZF(ZF_PLAIN, NX_NONE, 0);
            else if (mode == ZF_NU) SMO_ZF(ZF_NU, NX_NONE, 0);
            else if (mode == ZF_FWD_UPDATE) { if (next == NX_PLAIN) SMO_ZF(ZF_FWD_UPDATE, NX_PLAIN, 0); else SMO_ZF(ZF_FWD_UPDATE, NX_NONE, 0); }
            else { if (next == NX_CURL) SMO_ZF(ZF_ADJ_UPDATE, NX_CURL, 0); else SMO_ZF(ZF_ADJ_UPDATE, NX_NONE, 0); }
#undef SMO_ZF
            return SMO_OK;
        });
    }

    // ---- phases: everything between two slab exchanges (the exchange z-side <-> y-side is the host layer's job) -------
    bool in_tycache(int n) const { return d_tycache && sched.in_tycache(n, tycache_window, tycache_count); }
    cplx* tyslot(int n, int k = 0) {
        if (d_tystack) return d_tystack + (size_t)n * fld + (size_t)k * fldc;
        return d_tycache + (size_t)(n - sched.first(tycache_window)) * fld * nbatch() + (size_t)k * fldc;      // [slot][member][fld]
    }
    cplx* tyw(int f, int k) { return d_ty + (size_t)f * fld * nbatch() + (size_t)k * fldc; }       // work copy of Ty: field group f, chunk k
    bool have_ty(int n) const { return n >= 0 && n < cfg.n_iters && (d_tystack != nullptr || in_tycache(n)); }
    int fwd_A(int n) {
        if (zs_ready_fwd == n) { zs_ready_fwd = -1; return SMO_OK; }
        return z_inverse(ZI_PLAIN, snap(n), 0, 1);
    }
    int fwd_B(int n, int k) {
        cplx* ty = have_ty(n) ? tyslot(n, k) : tyw(0, k);
        SMO_TRY(y_pass(true, 0, 1, ty, k));
        SMO_TRY(x_pass(X_FUSED_FWD, k, nullptr, nullptr, ty));
        return y_pass(false, 0, 1, tyw(0, k), k);
    }
    int fwd_C(int n) {
        const bool fuse = fuse_next && n + 1 < cfg.n_iters;
        SMO_TRY(z_forward(ZF_FWD_UPDATE, snap(n + 1), snap(n), nullptr, fuse ? NX_PLAIN : NX_NONE));
        zs_ready_adj = -1;
        zs_ready_fwd = fuse ? n + 1 : -1;
        return SMO_OK;
    }
    int adj_init(int adjoint_type) {
        ScopedTimer t(timing, k_misc, stream);
        SMO_LAUNCH(kd_terminal, dim3(1024, cfg.batch), dim3(256), 0, stream, snap(cfg.n_iters), d_G, d_nu, g, cfg.cost == SMO_COST_INTEGRATED ? 1 : 0,
                           adjoint_type == SMO_ADJ_CONTINUOUS ? 1 : 0);
        if (d_acc) SMO_HIP(hipMemsetAsync(d_acc, 0, fld * nbatch() * sizeof(cplx), stream));      // (frozen velocity: neither nu^ nor the running sum)
        adj_cont = adjoint_type == SMO_ADJ_CONTINUOUS;
        zs_ready_fwd = zs_ready_adj = -1;
        return SMO_OK;
    }
    // inverse side of an adjoint step carries omega only (1 field group) when B_f was kept by the forward solve, else omega and B^_idx
    // (frozen velocity: omega only, always — B_f never enters the G^ recursion)
    int adj_groups(int idx) const { return (frozen_u || have_ty(idx)) ? 1 : 2; }
    // one slab, one chunk: field group 0 sits at the same place of the exchange buffer whether the step carries one group or two (zs_off: row + pos,
    // the second group tzc elements further), so the curl pass fused into the previous update serves a two-group step as well
    bool group0_layout_is_shared() const { return cfg.world == 1 && K == 1 && !force_exchange; }
    int adj_A(int idx) {
        const int nf = adj_groups(idx);
        if (zs_ready_adj == idx && (nf == 1 || group0_layout_is_shared())) {
            zs_ready_adj = -1;
            return nf == 2 ? z_inverse(ZI_PLAIN, snap(idx), 1, 2) : SMO_OK;      // (writes the second group only)
        }
        SMO_TRY(z_inverse(ZI_CURL, d_G, 0, nf));
        return nf == 2 ? z_inverse(ZI_PLAIN, snap(idx), 1, 2) : SMO_OK;
    }
    int adj_B(int idx, int k) {
        if (frozen_u) {
            SMO_TRY(y_pass(true, 0, 1, tyw(0, k), k));
            SMO_TRY(x_pass(X_FUSED_ADJ_B, k, nullptr, nullptr));
            return y_pass(false, 0, 1, tyw(0, k), k);
        }
        const int nf = adj_groups(idx);
        SMO_TRY(y_pass(true, 0, nf, tyw(0, k), k));
        if (nf == 2) SMO_TRY(y_pass(true, 1, 2, tyw(1, k), k));
        SMO_TRY(x_pass(X_FUSED_ADJ, k, nullptr, nullptr, nullptr, nf == 1 ? tyslot(idx, k) : nullptr));
        return y_pass(false, 0, 1, tyw(0, k), k);
    }
    int adj_C(int idx) {
        // the following adjoint step (index idx - 1) starts with the inverse z pass of curl(G^): fused when that step sends one field
        // group (same buffer layout as this kernel's input) and exists at all (the continuous sweep ends at index 1, the discrete at 0)
        const int nxt = idx - 1;
        const bool fuse = fuse_next && nxt >= (adj_cont ? 1 : 0) && (adj_groups(nxt) == 1 || group0_layout_is_shared());
        SMO_TRY(z_forward(ZF_ADJ_UPDATE, d_G, d_G, snap(idx), fuse ? NX_CURL : NX_NONE));
        zs_ready_fwd = -1;
        zs_ready_adj = fuse ? nxt : -1;
        return SMO_OK;
    }
    // The nu^ recursion of the reference, nu <- R nu - dt P F2_n (R = I - 2 k k^T/k^2, nu_N = 0), never leaves the solenoidal subspace,
    // where R is the identity: nu_0 = -dt P sum_n F2_n exactly.  The fused adjoint x pass therefore adds its second product
    // (curl G_n) x B_n, already transformed along x, to a running sum on the grid side (d_acc, the layout of Ty); the y and z passes,
    // the projection and the factor -dt are applied ONCE after the last step (nu_B / nu_C) instead of once per step: one y pass and
    // half a z pass less per adjoint step and, with slabs, one field group less to send back.
    int nu_B(int k) { return y_pass(false, 0, 1, d_acc + (size_t)k * fldc, k); }
    int nu_C() { return z_forward(ZF_NU, d_nu, nullptr, nullptr); }
    // grid vector (local slab of the flat X layout) -> truncated coefficients, in two phases around the exchange
    int g2c_A(const double* X, int k) { SMO_TRY(x_pass(X_FROM_GRID, k, X, nullptr)); return y_pass(false, 0, 1, tyw(0, k), k); }
    int g2c_C(cplx* out) { return z_forward(ZF_PLAIN, out, nullptr, nullptr); }
    // coefficients -> grid; scaled = multiply by dt*alpha(k) first ("undo LHS", FWD_Solve_KDyn.py:985-989)
    int c2g_A(const cplx* C, bool scaled) { return z_inverse(scaled ? ZI_SCALE : ZI_PLAIN, C, 0, 1); }
    int c2g_B(double* X, int k) { SMO_TRY(y_pass(true, 0, 1, tyw(0, k), k)); return x_pass(X_TO_GRID, k, nullptr, X); }   // X == nullptr: the U field

    size_t part_row() const { return n_part_rows * NPART; }     // doubles between the partial-sum rows of consecutive members
    // row 0 of every member's partials, each summed in index order -> out[0 .. batch-1]
    int reduce_partials(double* out) {
        SMO_HIP(hipMemcpy2DAsync(h_part.data(), NPART * sizeof(double), d_part, part_row() * sizeof(double), NPART * sizeof(double), nbatch(),
                                 hipMemcpyDeviceToHost, stream));
        SMO_HIP(hipStreamSynchronize(stream));
        for (size_t b = 0; b < nbatch(); ++b) {
            double s = 0.0;
            for (int i = 0; i < NPART; ++i) s += h_part[b * NPART + i];
            out[b] = s;
        }
        return SMO_OK;
    }
    int energy(const cplx* Bh, double* E) {            // this slab's share of sum_k w |B^|^2 (phase-level entry: batch 1)
        {
            ScopedTimer t(timing, k_misc, stream);
            SMO_LAUNCH(kd_energy, dim3(NPART), dim3(256), 0, stream, Bh, d_part, g, part_row());
        }
        return reduce_partials(E);
    }

    // ---- slab communicator: the pencil transposes and scalar reductions of the time loop, inside the library ------------------
    bool exchanging() const { return (cfg.world > 1 || force_exchange) && comm.ready(); }
    ~KDyn() override {
        (void)hipSetDevice(cfg.device);
        if (stream) (void)hipStreamSynchronize(stream);
        drop_graphs();
        if (cstream) { (void)hipStreamSynchronize(cstream); (void)hipStreamDestroy(cstream); }
        if (ev_main) (void)hipEventDestroy(ev_main);
        for (auto* v : {&ev_in, &ev_ph, &ev_out}) for (hipEvent_t e : *v) (void)hipEventDestroy(e);
    }
    // all-to-all of chunk k, nf field groups: z side -> y side (to_y) or back.  Peer blocks are contiguous: [chunk][peer][nf*tzc]
    // chained: an exchange of the time loop (stage()), whose send buffer is next written by the pull of the exchange that follows it on the
    // same stream — the multi-device transport then skips its second rendezvous (comm.hpp).  SMO_PEER_CHAINED=0 keeps the full protocol.
    int exchange(bool to_y, int nf, int k, hipStream_t s, bool chained = false) {
        if (!exchanging()) return SMO_OK;
        const size_t off = (size_t)k * (size_t)cfg.world * 2 * tzc;
        const cplx* src = (to_y ? zs : ys) + off;
        cplx* dst = (to_y ? ys : zs) + off;
        if (!to_y) zs_ready_fwd = zs_ready_adj = -1;
        ScopedTimer t(timing, k_ex, s);
        return comm.alltoall(src, dst, (size_t)nf * tzc * sizeof(cplx), s, chained && env.peer_chained);
    }
    enum { ST_FWD = 0, ST_ADJ = 1 };
    int grid_phase(int code, int idx, int k) { return code == ST_FWD ? fwd_B(idx, k) : adj_B(idx, k); }
    // one transpose -> grid work -> transpose back.  K > 1: chunk-pipelined — the K inbound exchanges are issued up front on the
    // communication stream, every chunk's grid kernels wait (stream-level, never the host) for their chunk only, and the outbound
    // exchange of chunk k overlaps the kernels of chunk k+1.
    int stage(int code, int idx, int nf_in, int nf_out) {
        if (!exchanging() || K == 1) {
            SMO_TRY(exchange(true, nf_in, 0, stream, true));
            SMO_TRY(grid_phase(code, idx, 0));
            return exchange(false, nf_out, 0, stream, true);
        }
        SMO_HIP(hipEventRecord(ev_main, stream));
        SMO_HIP(hipStreamWaitEvent(cstream, ev_main, 0));
        for (int k = 0; k < K; ++k) {
            SMO_TRY(exchange(true, nf_in, k, cstream, true));
            SMO_HIP(hipEventRecord(ev_in[k], cstream));
        }
        for (int k = 0; k < K; ++k) {
            SMO_HIP(hipStreamWaitEvent(stream, ev_in[k], 0));
            SMO_TRY(grid_phase(code, idx, k));
            SMO_HIP(hipEventRecord(ev_ph[k], stream));
            SMO_HIP(hipStreamWaitEvent(cstream, ev_ph[k], 0));
            SMO_TRY(exchange(false, nf_out, k, cstream, true));
            SMO_HIP(hipEventRecord(ev_out[k], cstream));
        }
        for (int k = 0; k < K; ++k) SMO_HIP(hipStreamWaitEvent(stream, ev_out[k], 0));
        return SMO_OK;
    }
    // keep = false: recomputation of a window (checkpointing): the grid-side state of step n is not kept again
    int step_fwd(int n, bool keep) {
        act_now = cfg.n_iters - n;                          // members with a shorter horizon idle through this step (Geom::act)
        int rc = fwd_A(n);
        if (rc == SMO_OK) rc = stage(ST_FWD, keep ? n : -1, 1, 1);
        if (rc == SMO_OK) rc = fwd_C(n);
        act_now = 0;
        return rc;
    }
    int grid_to_coeff(const double* X, cplx* out) {
        for (int k = 0; k < K; ++k) { SMO_TRY(g2c_A(X, k)); SMO_TRY(exchange(false, 1, k, stream)); }
        return g2c_C(out);
    }
    int coeff_to_grid(const cplx* C, bool scaled, double* X) {
        SMO_TRY(c2g_A(C, scaled));
        for (int k = 0; k < K; ++k) { SMO_TRY(exchange(true, 1, k, stream)); SMO_TRY(c2g_B(X, k)); }
        return SMO_OK;
    }
    int allreduce(double* v, int n) { return cfg.world > 1 ? comm.allreduce_sum(v, n, stream, d_red) : SMO_OK; }

    // Called once the transport exists (collective): the ranks agree on what each of them decided from its own free HBM — the
    // checkpoint interval and whether the grid-side states are kept (that fixes how many field groups an adjoint step sends) —
    // before the first exchange could mismatch, and the chunk pipeline is set up.
    // stream and events of the chunk pipeline, for the current K
    int pipeline_resources() {
        if (!cstream) SMO_HIP(hipStreamCreateWithFlags(&cstream, hipStreamNonBlocking));
        if (!ev_main) SMO_HIP(hipEventCreateWithFlags(&ev_main, hipEventDisableTiming));
        for (auto* vec : {&ev_in, &ev_ph, &ev_out})
            while ((int)vec->size() < K) { hipEvent_t e; SMO_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); vec->push_back(e); }
        return SMO_OK;
    }
    int comm_attach() {
        const int ck = sched.ck;
        double v[4] = {d_tystack ? 1.0 : 0.0, (double)ck, (double)ck * ck, d_tycache ? 1.0 : 0.0};
        SMO_TRY(allreduce(v, 4));
        const double W = cfg.world;
        if (std::fabs(W * v[2] - v[1] * v[1]) > 0.5) {
            set_error("KDYN: the ranks chose different checkpoint intervals from their free HBM (mine: %d); pass an explicit smo_config.ckpt", ck);
            return SMO_ERR_STATE;
        }
        if (d_tystack && v[0] < W - 0.5) {               // some rank could not keep the grid-side states: nobody does
            SMO_HIP(hipStreamSynchronize(stream));
            SMO_TRY(pool.free_one(d_tystack));
            stack_bytes -= (size_t)cfg.n_iters * fld * sizeof(cplx);
            d_tystack = nullptr;
        }
        if (d_tycache && v[3] < W - 0.5) {                // the same for the Ty cache of the checkpoint windows
            SMO_HIP(hipStreamSynchronize(stream));
            SMO_TRY(pool.free_one(d_tycache));
            d_tycache = nullptr; tycache_window = -1;
        }
        int k = env_int("SMO_SLAB_CHUNKS", 0);           // read here, not at creation: a host layer may set it between the two
        // default: up to 4 chunks of at least 36864 (y,z) points (one 192 x 192 plane set).  Chunking is not free: with the null transport
        // (no exchange at all) the 256^3 step pair of an 8-way decomposition takes 570 us with one chunk and 739 us with two, 1075 / 1390 us
        // 4-way with 1 / 4 (profiles/r03_slab_geometry_256.jsonl) — smaller kernels fill the GPU worse (a fused x pass of 9216 points is
        // 1152 tiles for 1024 slots) and every chunk adds event traffic — so it only pays where the transposes are slow enough to be worth
        // hiding, which a one-GPU measurement cannot tell: LibSlabKDyn.autotune_chunks / SMO_SLAB_CHUNKS decide on the node itself.
        if (k <= 0) k = cfg.world > 1 ? std::max(1, std::min(4, (int)(((size_t)g.G * g.Gzr) / 36864))) : 1;
        while (k > 1 && (g.Gzr % k || (g.Gzr / k) % 2 || ((size_t)g.G * (g.Gzr / k)) % 4)) --k;
        if (k != K) SMO_TRY(set_chunks(k));
        SMO_TRY(pipeline_resources());
        have_forward = false;
        return SMO_OK;
    }
    // a context whose ranks could not agree (different checkpoint intervals, a buffer that would not free, chunks that do not divide)
    // must not keep a live transport: K, the Ty stack and the Ty cache may then differ between the ranks and the next solve would hang
    // in a mismatched all-to-all.  The transport is dropped, smo_forward fails with SMO_ERR_STATE, and smo_comm_init may be called again.
    int attach_or_drop() {
        const int rc = comm_attach();
        if (rc != SMO_OK) {
            const std::string why = last_error();
            (void)hipStreamSynchronize(stream);
            comm.reset();
            set_error("%s (the communicator was dropped: call smo_comm_init / smo_comm_set_transport again once the ranks agree)", why.c_str());
        }
        return rc;
    }
    int comm_init(const void* id128) override {
        if (cfg.world == 1 && !force_exchange) { set_error("smo_comm_init: single-slab context (nothing to exchange)"); return SMO_ERR_STATE; }
        SMO_TRY(comm.init_rccl(cfg.rank, cfg.world, id128));
        return attach_or_drop();
    }
    int comm_set_transport(smo_alltoall_fn a2a, smo_allreduce_fn ared, void* user) override {
        if (cfg.world == 1 && !force_exchange) { set_error("smo_comm_set_transport: single-slab context (nothing to exchange)"); return SMO_ERR_STATE; }
        SMO_TRY(comm.set_transport(cfg.rank, cfg.world, a2a, ared, user));
        return attach_or_drop();
    }
    int comm_set_peers(PeerGroup* grp, int rank) override {
        if (cfg.world == 1 && !force_exchange) { set_error("comm_set_peers: single-slab context (nothing to exchange)"); return SMO_ERR_STATE; }
        if (rank != cfg.rank || grp->world() != cfg.world) { set_error("comm_set_peers: rank %d of %d does not match the context (%d of %d)", rank, grp->world(), cfg.rank, cfg.world); return SMO_ERR_ARG; }
        SMO_TRY(comm.set_peers(rank, grp));
        return attach_or_drop();
    }
    double comm_info(int key) const override {
        if (key == 0) return (double)K;
        if (key == 1) return 3.0 + (d_tystack ? 1.0 : 2.0);
        if (key == 2) return comm.is_rccl() ? 1.0 : 0.0;
        return 0.0;                               // keys 3, 4: the multi-device context's transport (csrc/multi.cpp)
    }

    // ---- the three callbacks: phases back to back; with slabs the transposes in between go through the communicator ------------
    int loop_ok(const char* who) {
        if ((cfg.world > 1 || force_exchange) && !comm.ready()) {
            set_error("%s: %d slabs and no communicator — call smo_comm_init (RCCL) or smo_comm_set_transport first, or drive the phases "
                      "yourself (smo_kdyn_op)", who, cfg.world);
            return SMO_ERR_STATE;
        }
        if (K != 1 && !exchanging()) { set_error("%s: the z slab is cut into %d chunks (phase-level use only)", who, K); return SMO_ERR_STATE; }
        return need_buffers();
    }
    // ---- HIP graphs for the launch-bound sizes ----------------------------------------------------------------------------
    // A 24^3 solve (the reference script's default) is 2000 steps x 4 kernels of ~2 us of work each: 4.8 us per launch measured.  For
    // such grids on one GPU the whole forward solve and the whole adjoint sweep are captured ONCE as HIP graphs (the stack addresses
    // never change; the caller's vectors are copied to / from fixed buffers so that the graphs are independent of them) and replayed
    // by every later call.  Same kernels in the same order: results are bit-identical with the launch-by-launch path (SMO_KD_GRAPH=0).
    // Measured (tools/time_small_grid.py, profiles/r02_small_grid_graph.jsonl): 77.0 -> 68.7 ms per gradient at 24^3 (4.8 -> 4.3 us per
    // kernel: what remains is the GPU-side hand-over between dependent kernels, not the host), no gain from 32^3 up, +75 ms for the
    // capture at the first call — hence on by default only up to G = 36.  Off while kernel timing is on, with slabs, chunks or
    // checkpoint windows.
    bool use_graph() const {
        if (graph_broken || env.graph == 0 || timing.on || cfg.world != 1 || force_exchange || K != 1 || sched.ck != 1) return false;
        if (cfg.n_iters > 8192) return false;                 // a graph holds ~4 nodes per step: keep its instantiation in the tens of milliseconds
        return env.graph == 1 || g.G <= env.graph_maxg;
    }
    template <class F> int run_graph(hipGraphExec_t* gx, Flags* after, F enqueue) {
        if (!*gx) {
            hipGraph_t graph = nullptr;
            SMO_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
            const int rc = enqueue();
            const hipError_t e = hipStreamEndCapture(stream, &graph);
            if (rc != SMO_OK || e != hipSuccess || !graph) {
                if (graph) (void)hipGraphDestroy(graph);
                (void)hipGetLastError();
                graph_broken = true;                     // this context goes on launch by launch
                return rc != SMO_OK ? rc : enqueue();
            }
            const hipError_t ei = hipGraphInstantiate(gx, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (ei != hipSuccess) { *gx = nullptr; (void)hipGetLastError(); graph_broken = true; return enqueue(); }
            *after = Flags{zs_ready_fwd, zs_ready_adj, adj_cont};
        }
        SMO_HIP(hipGraphLaunch(*gx, stream));
        zs_ready_fwd = after->zf; zs_ready_adj = after->za; adj_cont = after->cont;      // what the enqueueing code leaves behind
        ++graph_replays;
        return SMO_OK;
    }
    int n_grads() const override { return frozen_u ? 1 : 2; }
    int graph_buffers() {
        for (int c = 0; c < 2; ++c) {
            if (!d_xin[c]) SMO_TRY(pool.alloc(&d_xin[c], n_grid * nbatch()));
            if (c < n_grads() && !d_gout[c]) SMO_TRY(pool.alloc(&d_gout[c], n_grid * nbatch()));
        }
        return SMO_OK;
    }
    void drop_graphs() {
        for (hipGraphExec_t* x : {&gx_fwd, &gx_adj[0], &gx_adj[1]})
            if (*x) { (void)hipGraphExecDestroy(*x); *x = nullptr; }
    }

    // everything of a forward solve that is a kernel launch (the partial sums of J stay in d_part)
    int fwd_enqueue(const double* B, const double* U) {
        const int N = cfg.n_iters;
        tycache_window = -1;                               // the states change: whatever the last adjoint sweep cached is stale
        act_now = 0;
        const bool integ = cfg.cost == SMO_COST_INTEGRATED;
        // U: truncate to the retained modes, back to the grid (NCC fields are band-limited by the solver)
        SMO_TRY(grid_to_coeff(U, d_G));
        SMO_TRY(coeff_to_grid(d_G, false, nullptr));
        SMO_TRY(grid_to_coeff(B, snap(0)));
        for (int n = 0; n < N; ++n) {
            if (integ) {                                   // <B_n,B_n> partial sums stay on the device until the end of the solve
                ScopedTimer t(timing, k_misc, stream);
                SMO_LAUNCH(kd_energy, dim3(NPART, cfg.batch), dim3(256), 0, stream, snap(n), d_part + (size_t)n * NPART, g, part_row());
            }
            SMO_TRY(step_fwd(n, true));
        }
        ScopedTimer t(timing, k_misc, stream);
        SMO_LAUNCH(kd_energy, dim3(NPART, cfg.batch), dim3(256), 0, stream, snap(N), d_part + (integ ? (size_t)N * NPART : 0), g, part_row());
        return SMO_OK;
    }
    static double now_ms() { return 1e-6 * (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    int forward_dev(const double* const* X, double* J) override {
        SMO_TRY(loop_ok("smo_forward"));
        have_forward = false;
        const double t_in = now_ms(), w_in = comm.wait_ms();
        const int N = cfg.n_iters;
        const bool integ = cfg.cost == SMO_COST_INTEGRATED;
        if (use_graph()) {
            SMO_TRY(graph_buffers());
            for (int c = 0; c < 2; ++c) SMO_HIP(hipMemcpyAsync(d_xin[c], X[c], n_grid * nbatch() * sizeof(double), hipMemcpyDeviceToDevice, stream));
            SMO_TRY(run_graph(&gx_fwd, &fl_fwd, [&]() { return fwd_enqueue(d_xin[0], d_xin[1]); }));
        } else {
            SMO_TRY(fwd_enqueue(X[0], X[1]));
        }
        issue_ms_fwd = (now_ms() - t_in) - (comm.wait_ms() - w_in);
        scratch_window = sched.window_after_forward();
        const size_t rows = integ ? (size_t)N + 1 : 1;      // (= n_part_rows)
        SMO_HIP(hipMemcpyAsync(h_part.data(), d_part, nbatch() * rows * NPART * sizeof(double), hipMemcpyDeviceToHost, stream));
        SMO_HIP(hipStreamSynchronize(stream));
        SMO_HIP(hipGetLastError());
        for (size_t b = 0; b < nbatch(); ++b) {               // each member: its own rows, in the order of a batch-1 solve
            const double* hp = h_part.data() + b * part_row();
            double Jacc = 0.0;
            // (a member with its own horizon: the rows of its own states s_b ... N, the sequence of a batch-1 solve of N_b steps)
            for (size_t n = integ ? (size_t)first_state(b) : 0; n < rows; ++n) {
                double e = 0.0;
                for (int i = 0; i < NPART; ++i) e += hp[n * NPART + i];
                Jacc += integ ? cfg.dt * e : e;
            }
            SMO_TRY(allreduce(&Jacc, 1));                    // slabs (batch 1): every rank holds its share of the spectral sum
            J[b] = -Jacc;
        }
        SMO_HIP(hipStreamSynchronize(stream));
        if (cstream) SMO_HIP(hipStreamSynchronize(cstream));
        have_forward = true;
        return SMO_OK;
    }

    int adj_enqueue(int adjoint_type, double* gB, double* gU) {
        const int N = cfg.n_iters;
        const bool cont = adjoint_type == SMO_ADJ_CONTINUOUS;
        act_now = 0;
        SMO_TRY(ensure(N));
        SMO_TRY(adj_init(adjoint_type));
        int idx = cont ? N : N - 1;
        // frozen velocity, Final cost: the sweep reads no forward state but B^_N, so no window is ever replayed; Integrated keeps ensure()
        // because its z update reads snap(idx)
        const bool states = !frozen_u || cfg.cost == SMO_COST_INTEGRATED;
        for (int it = 0; it < N; ++it, --idx) {
            if (states) SMO_TRY(ensure(idx));
            // members whose own sweep is over (N_b steps) sit this iteration out (Geom::act): the discrete sweep visits idx = N-1 ... 0, the
            // continuous one idx = N ... 1, and either way iteration `it` belongs to the members with N_b >= it + 1
            act_now = cont ? N - idx + 1 : N - idx;
            int rc = adj_A(idx);
            if (rc == SMO_OK) rc = stage(ST_ADJ, idx, adj_groups(idx), 1);
            if (rc == SMO_OK) rc = adj_C(idx);
            act_now = 0;
            SMO_TRY(rc);
        }
        SMO_TRY(coeff_to_grid(d_G, !cont, gB));
        if (frozen_u) return SMO_OK;                      // no nu^, no dJ/dU: gU is never written
        for (int k = 0; k < K; ++k) { SMO_TRY(nu_B(k)); SMO_TRY(exchange(false, 1, k, stream)); }
        SMO_TRY(nu_C());
        return coeff_to_grid(d_nu, false, gU);
    }
    int adjoint_dev(const double* const*, int adjoint_type, double* const* grad) override {
        SMO_TRY(loop_ok("smo_adjoint"));
        const double t_in = now_ms(), w_in = comm.wait_ms();
        if (use_graph()) {
            SMO_TRY(graph_buffers());
            const int a = adjoint_type == SMO_ADJ_CONTINUOUS ? 1 : 0;
            SMO_TRY(run_graph(&gx_adj[a], &fl_adj[a], [&]() { return adj_enqueue(adjoint_type, d_gout[0], d_gout[1]); }));
            for (int c = 0; c < n_grads(); ++c) SMO_HIP(hipMemcpyAsync(grad[c], d_gout[c], n_grid * nbatch() * sizeof(double), hipMemcpyDeviceToDevice, stream));
        } else {
            SMO_TRY(adj_enqueue(adjoint_type, grad[0], frozen_u ? nullptr : grad[1]));
        }
        issue_ms_adj = (now_ms() - t_in) - (comm.wait_ms() - w_in);
        SMO_HIP(hipGetLastError());
        SMO_HIP(hipStreamSynchronize(stream));
        if (cstream) SMO_HIP(hipStreamSynchronize(cstream));
        return SMO_OK;
    }

    int inner_dev(const double* x, const double* y, double* out) override {       // <x,y>; slabs without a communicator: this slab's share
        {   // (batch: one value per member, vectors [batch][n_grid])
            ScopedTimer t(timing, k_dot, stream, true);
            SMO_LAUNCH_T(t, kd_dot, dim3(NPART, cfg.batch), dim3(256), 0, stream, x, y, d_part, n_grid, part_row());
        }
        SMO_HIP(hipGetLastError());
        SMO_TRY(reduce_partials(out));
        for (size_t b = 0; b < nbatch(); ++b) {
            if (comm.ready()) SMO_TRY(allreduce(&out[b], 1));
            out[b] = out[b] / ((double)g.G * g.G * g.G);
        }
        return SMO_OK;
    }

    double info(int key) const override {
        if (key == 0) return sched.pingpong ? (double)cfg.n_iters : (double)sched.ck;
        if (key == 6) return frozen_u ? 1.0 : 0.0;
        if (key == 7) return (double)wt_mask;
        if (key == 2) return (double)graph_replays;
        if (key == 3) return (double)g.tyl;
        if (key == 4) return issue_ms_fwd + issue_ms_adj;
        if (key == 5) return sched.has_tail() ? (double)sched.dense_from : -1.0;
        return d_tystack ? (double)((size_t)cfg.n_iters * fld * sizeof(cplx)) : 0.0;
    }

    // smo_transform for the 3-D case (host buffers): which = 0: three grid fields float64[3][G][G][G] -> their truncated coefficients
    // complex128[3][a][m][m] (Dedalus' amplitude normalisation); which = 1: the inverse.  The same passes the solves use; single GPU.
    int transform_host(int which, const double* in, double* out) override {
        if (cfg.world != 1 || K != 1) { set_error("smo_transform (KDYN): single-GPU contexts only"); return SMO_ERR_UNSUPPORTED; }
        if (cfg.batch != 1) { set_error("smo_transform (KDYN): not available on a batched context (batch = %d): use a batch-1 context", cfg.batch); return SMO_ERR_UNSUPPORTED; }
        if (which != 0 && which != 1) { set_error("smo_transform (KDYN): which = 0 (grid -> coefficients) or 1 (coefficients -> grid)"); return SMO_ERR_ARG; }
        if (!d_tgrid) SMO_TRY(pool.alloc(&d_tgrid, n_grid));
        have_forward = false;                               // d_G (the adjoint's state) is the scratch spectrum here
        if (which == 0) {
            SMO_HIP(hipMemcpyAsync(d_tgrid, in, n_grid * sizeof(double), hipMemcpyHostToDevice, stream));
            SMO_TRY(grid_to_coeff(d_tgrid, d_G));
            SMO_HIP(hipMemcpyAsync(out, d_G, 3 * nmode * sizeof(cplx), hipMemcpyDeviceToHost, stream));
        } else {
            SMO_HIP(hipMemcpyAsync(d_G, in, 3 * nmode * sizeof(cplx), hipMemcpyHostToDevice, stream));
            SMO_TRY(coeff_to_grid(d_G, false, d_tgrid));
            SMO_HIP(hipMemcpyAsync(out, d_tgrid, n_grid * sizeof(double), hipMemcpyDeviceToHost, stream));
        }
        SMO_HIP(hipGetLastError());
        SMO_HIP(hipStreamSynchronize(stream));
        return SMO_OK;
    }

    int snapshot_read(int b, int index, double* out) override {       // member b (the window is recomputed for all members at once)
        const int last = cfg.n_iters - first_state((size_t)b);      // the member's own horizon: `index` counts its own time
        if (sched.pingpong && index != last) {
            set_error("smo_snapshot_read: snapshot %d is not kept: the context was created with keep_states = 0 and holds state %d only", index, last);
            return SMO_ERR_STATE;
        }
        index += first_state((size_t)b);
        SMO_TRY(ensure(index));
        SMO_HIP(hipMemcpyAsync(out, snap(index) + (size_t)b * g.mc, 3 * nmode * sizeof(cplx), hipMemcpyDeviceToHost, stream));
        SMO_HIP(hipStreamSynchronize(stream));
        return SMO_OK;
    }

    // ---- phase-level entry for the slab-decomposed driver (smo_kdyn_op) -------------------------------------------------
    int kdyn_op(int op, int i0, int i1, void* p0, void* p1, double* out) override {
        if (frozen_u) { set_error("smo_kdyn_op: not available on a frozen-velocity context (smo_create_frozen_u: one GPU, no phase-level entry)"); return SMO_ERR_UNSUPPORTED; }
        if (cfg.batch != 1) { set_error("smo_kdyn_op: not available on a batched context (batch = %d)", cfg.batch); return SMO_ERR_UNSUPPORTED; }
        if (!horizons.empty()) { set_error("smo_kdyn_op: not available while horizons are set (smo_set_horizons(ctx, NULL) removes them)"); return SMO_ERR_UNSUPPORTED; }
        if (op == SMO_KD_SET_CHUNKS) {                       // also on a context that runs the loop itself: re-tune the exchange pipeline
            SMO_HIP(hipStreamSynchronize(stream));
            if (cstream) SMO_HIP(hipStreamSynchronize(cstream));
            SMO_TRY(set_chunks(i0));
            return comm.ready() ? pipeline_resources() : SMO_OK;
        }
        if (op == SMO_KD_SET_BUFFERS) {
            if (!p0 || !p1) { set_error("SMO_KD_SET_BUFFERS: null buffer"); return SMO_ERR_ARG; }
            zs = static_cast<cplx*>(p0); ys = static_cast<cplx*>(p1); zs_ready_fwd = zs_ready_adj = -1;
            drop_graphs();
            return SMO_OK;
        }
        if (op == SMO_KD_EXCHANGE_ELEMS) { if (!out) return SMO_ERR_ARG; *out = (double)(tzb * cfg.world); return SMO_OK; }
        SMO_TRY(need_buffers());
        const int N = cfg.n_iters;
        auto chunk_ok = [&](int k) { if (k < 0 || k >= K) { set_error("smo_kdyn_op(%d): chunk %d out of range (%d chunks)", op, k, K); return false; } return true; };
        auto step_ok = [&](int n, int hi) { if (n < 0 || n > hi) { set_error("smo_kdyn_op(%d): index %d out of range", op, n); return false; } return true; };
        int rc = SMO_OK;
        switch (op) {
            case SMO_KD_G2C_A: if (!p0 || !chunk_ok(i1)) return SMO_ERR_ARG; rc = g2c_A(static_cast<const double*>(p0), i1); break;
            case SMO_KD_G2C_C: rc = g2c_C(i0 == 0 ? snap(0) : d_G); if (i0 == 0) have_forward = false; break;
            case SMO_KD_C2G_A: rc = c2g_A(i0 == 2 ? d_nu : d_G, i0 == 0); break;
            case SMO_KD_C2G_B: if (!chunk_ok(i1)) return SMO_ERR_ARG; rc = c2g_B(static_cast<double*>(p0), i1); break;
            case SMO_KD_FWD_A: if (!step_ok(i0, N - 1)) return SMO_ERR_ARG; rc = fwd_A(i0); break;
            case SMO_KD_FWD_B: if (!chunk_ok(i1)) return SMO_ERR_ARG; rc = fwd_B(i0, i1); break;
            case SMO_KD_FWD_C: if (!step_ok(i0, N - 1)) return SMO_ERR_ARG; rc = fwd_C(i0); if (i0 == N - 1) have_forward = true; break;
            case SMO_KD_ENERGY: if (!step_ok(i0, N) || !out) return SMO_ERR_ARG; return energy(snap(i0), out);
            case SMO_KD_ADJ_INIT:
                if (!have_forward) { set_error("smo_kdyn_op: adjoint before forward"); return SMO_ERR_STATE; }
                rc = adj_init(i0); break;
            case SMO_KD_ADJ_A: if (!step_ok(i0, N)) return SMO_ERR_ARG; rc = adj_A(i0); break;
            case SMO_KD_ADJ_B: if (!step_ok(i0, N) || !chunk_ok(i1)) return SMO_ERR_ARG; rc = adj_B(i0, i1); break;
            case SMO_KD_ADJ_C: if (!step_ok(i0, N)) return SMO_ERR_ARG; rc = adj_C(i0); break;
            case SMO_KD_NU_B: if (!chunk_ok(i1)) return SMO_ERR_ARG; rc = nu_B(i1); break;
            case SMO_KD_NU_C: rc = nu_C(); break;
            case SMO_KD_SYNC: SMO_HIP(hipStreamSynchronize(stream)); break;
            default: set_error("smo_kdyn_op: unknown op %d", op); return SMO_ERR_ARG;
        }
        if (rc == SMO_OK) SMO_HIP(hipGetLastError());
        return rc;
    }
};

}  // namespace

Context* make_kdyn(const smo_config& cfg) { return new KDyn(cfg); }

}  // namespace smo
