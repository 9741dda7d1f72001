// Cross-member block operations of a batched context (include/smo.h: smo_gram*, smo_combine*).
//
// A batched context holds B vectors of n doubles each ([B][n], member stride n).  Everything else the library offers treats the members as
// independent problems; these two kernels are the operations in which member a meets member b:
//
//   block_gram     G[a][b] = (sum_k x_a[k] y_b[k]) / scale        [B x n] . [n x B]   (scale: the context's inner product, KDYN G^3, SH23 G)
//   block_combine  out_b[k] = sum_a C[a][b] x_a[k]                [n x B] . [B x B]
//
// Both are tall-skinny fp64 GEMMs that should cost one pass over their operands.
//   block_gram: a workgroup owns a contiguous range of element chunks (blockops_tiles.hpp).  Per chunk it loads every member's piece
//     coalesced (16-byte loads where the member is 16-byte aligned, two 8-byte loads otherwise, nothing beyond n and no padded member), stages it
//     in LDS and feeds v_mfma_f64_16x16x4_f64 from there; the four waves split the chunk's k steps and each keeps all (<= 16) tiles of the
//     64 x 64 block.  The chunk length follows the member count, so that a workgroup has about 16 KB per operand in flight, and the next chunk
//     is requested before the current one is multiplied.  At the end the waves add their tiles in LDS in wave order and the workgroup writes
//     ONE partial block; block_gram_finish adds the partial blocks in a fixed order and divides once.  No atomics: the same input gives the
//     same bits.
//   block_combine: fp64 MFMA has no rate advantage over the vector unit on gfx950 and this product needs no reduction across lanes, so a lane
//     owns one element k, reads x_a[k] for a = 0, 1, ... (a wave reads 512 contiguous bytes per member, eight members ahead) and keeps up to
//     64 outputs in registers; the coefficients sit in LDS and are read as broadcasts.  The sum over a is an fma chain in ascending a
//     starting from +0.
#include <algorithm>
#include <cstdint>

#include "blockops_tiles.hpp"
#include "smo_common.hpp"

namespace smo {
namespace {

using namespace blockops;
typedef double v4d __attribute__((ext_vector_type(4)));

// one operand's loads of one chunk into registers: v[p] = the element pair of item (p, lane); padding stays zero and is never read
template <int KC>
__device__ __forceinline__ void gram_fetch(double2 (&v)[max_passes(KC)], const GramPlan& p, const double* __restrict__ base, int rows, size_t chunk, int lane) {
#pragma unroll
    for (int ps = 0; ps < max_passes(KC); ++ps) {
        v[ps] = make_double2(0.0, 0.0);
        const GramItem it = gram_item(p, chunk, ps, lane);
        if (row_is_padding(it.row, rows) || elem_is_padding(it.k, p.n)) continue;
        const double* src = base + (size_t)it.row * p.n + it.k;
        if (!elem_is_padding(it.k + 1, p.n)) {
            if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) v[ps] = *reinterpret_cast<const double2*>(src);
            else { v[ps].x = src[0]; v[ps].y = src[1]; }
        } else {
            v[ps].x = src[0];
        }
    }
}
template <int KC>
__device__ __forceinline__ void gram_stage(double* __restrict__ dst, const double2 (&v)[max_passes(KC)], const GramPlan& p, int rows, int lane) {
#pragma unroll
    for (int ps = 0; ps < max_passes(KC); ++ps) {
        const GramItem it = gram_item(p, 0, ps, lane);
        if (row_is_padding(it.row, rows)) continue;
        *reinterpret_cast<double2*>(dst + it.row * lds_stride(KC) + it.col) = v[ps];
    }
}

// grid (nwg, row block, column block); sym: y == x — blocks below the diagonal leave at entry, a diagonal block stages x alone and computes the
// tiles on and above the diagonal.  partial: [nwg][B][B].
template <int NT, int KC>
__global__ __launch_bounds__(256) void block_gram(const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ partial, GramPlan p, int sym) {
    constexpr int S = lds_stride(KC), LROWS = lds_rows(KC), ROWS = kTile * NT;
    static_assert(ROWS * ROWS <= 2 * LROWS * S && ROWS <= LROWS + kTile - 1, "the reduction image must fit the staging buffers");
    __shared__ __attribute__((aligned(16))) double lds[2 * LROWS * S];
    double* xs = lds;
    double* ys = lds + LROWS * S;
    const int rb = blockIdx.y, cb = blockIdx.z;
    if (sym && cb < rb) return;
    const bool diag = sym && rb == cb;
    const int rows_x = block_rows(p, rb), rows_y = block_rows(p, cb);
    const double* xb = x + (size_t)rb * kBlock * p.n;
    const double* yb = y + (size_t)cb * kBlock * p.n;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    p.nt = NT; p.kc = KC;                                                      // (what the host put there: lets the item arithmetic fold to shifts)

    for (int i = tid; i < 2 * LROWS * S; i += kThreads) lds[i] = 0.0;         // the zero row (and the tail of the last chunk) stay zero

    v4d acc[NT][NT];
#pragma unroll
    for (int r = 0; r < NT; ++r)
#pragma unroll
        for (int c = 0; c < NT; ++c) acc[r][c] = (v4d){0.0, 0.0, 0.0, 0.0};

    const double* bs = diag ? xs : ys;
    // the next chunk's loads are in flight while this chunk's MFMAs run
    double2 vx[max_passes(KC)], vy[max_passes(KC)];
    const size_t first = (size_t)blockIdx.x * p.cpw, last = (first + p.cpw < p.nchunks) ? first + p.cpw : p.nchunks;
    if (first < last) {
        gram_fetch<KC>(vx, p, xb, rows_x, first, tid);
        if (!diag) gram_fetch<KC>(vy, p, yb, rows_y, first, tid);
    }
    for (size_t chunk = first; chunk < last; ++chunk) {
        __syncthreads();                                                       // the previous chunk's operand reads (first pass: the zero fill)
        gram_stage<KC>(xs, vx, p, rows_x, tid);
        if (!diag) gram_stage<KC>(ys, vy, p, rows_y, tid);
        __syncthreads();
        if (chunk + 1 < last) {
            gram_fetch<KC>(vx, p, xb, rows_x, chunk + 1, tid);
            if (!diag) gram_fetch<KC>(vy, p, yb, rows_y, chunk + 1, tid);
        }
#pragma unroll 8
        for (int s0 = 0; s0 < KC / kKStep; s0 += kWaves) {                     // wave w takes the k steps w, w + 4, ...
            const int s = s0 + wave;
            double a[NT], b[NT];
            const int col = mfma_col(s, lane);
#pragma unroll
            for (int r = 0; r < NT; ++r) a[r] = xs[lds_row(mfma_row(r, lane), rows_x, KC) * S + col];
#pragma unroll
            for (int c = 0; c < NT; ++c) b[c] = bs[lds_row(mfma_row(c, lane), rows_y, KC) * S + col];
#pragma unroll
            for (int r = 0; r < NT; ++r)
#pragma unroll
                for (int c = 0; c < NT; ++c)
                    if (!diag || c >= r) acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[r], b[c], acc[r][c], 0, 0, 0);
        }
    }

    // the four waves' tiles, added in wave order in an LDS image [ROWS][ROWS] of the block
    double* red = lds;
    for (int w = 0; w < kWaves; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int r = 0; r < NT; ++r)
#pragma unroll
                for (int c = 0; c < NT; ++c)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int idx = (kTile * r + acc_row(lane, v)) * ROWS + kTile * c + acc_col(lane);
                        red[idx] = (w == 0) ? acc[r][c][v] : red[idx] + acc[r][c][v];
                    }
        }
    }
    __syncthreads();
    double* pb = partial + (size_t)blockIdx.x * p.B * p.B;
    for (int i = tid; i < ROWS * ROWS; i += kThreads) {
        const int r = i / ROWS, c = i % ROWS;
        if (r < rows_x && c < rows_y) pb[(size_t)(rb * kBlock + r) * p.B + cb * kBlock + c] = red[i];
    }
}

// out[a][b] = (sum over the workgroups of partial[w][a][b]) / scale in a fixed order: 8 entries per workgroup, the workgroup range cut into 32
// contiguous slices that are summed in ascending w by one lane each and then added in ascending slice order.  sym: the entries below the
// diagonal take the sums of their mirror images, term for term.
__global__ __launch_bounds__(256) void block_gram_finish(const double* __restrict__ partial, double* __restrict__ out, int B, int nwg, double scale, int sym) {
    __shared__ double part[32][8];
    const int e = threadIdx.x & 7, sl = threadIdx.x >> 3;
    const int i = blockIdx.x * 8 + e;
    double acc = 0.0;
    if (i < B * B) {
        int a = i / B, b = i % B;
        if (sym && a > b) { const int t = a; a = b; b = t; }
        const int per = (nwg + 31) / 32, w0 = sl * per, w1 = (w0 + per < nwg) ? w0 + per : nwg;
        const double* src = partial + (size_t)a * B + b;
#pragma unroll 4
        for (int w = w0; w < w1; ++w) acc += src[(size_t)w * B * B];
    }
    part[sl][e] = acc;
    __syncthreads();
    if (sl == 0 && i < B * B) {
        double t = part[0][e];
        for (int q = 1; q < 32; ++q) t += part[q][e];
        out[i] = t / scale;
    }
}

// grid (element workgroups striding the 256-element tiles, column blocks of NB outputs); Cp: [B][ldc], zero beyond column B.  The coefficients
// of up to 64 input members sit in LDS ([a][NB], read as broadcasts); beyond 64 members they are reloaded per block of 64 inputs.
template <int NB>
__global__ __launch_bounds__(256) void block_combine(const double* __restrict__ x, const double* __restrict__ Cp, double* __restrict__ out, int B, size_t n, int ldc,
                                                     size_t ntiles) {
    __shared__ __attribute__((aligned(16))) double cs[kBlock * NB];
    const int b0 = blockIdx.y * NB;
    const bool reload = B > kBlock;
    if (!reload) {
        for (int i = threadIdx.x; i < B * NB; i += kThreads) cs[i] = Cp[(size_t)(i / NB) * ldc + b0 + i % NB];
        __syncthreads();
    }
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t k = combine_elem(tile, threadIdx.x);
        const bool valid = !elem_is_padding(k, n);
        double acc[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = 0.0;
        for (int a0 = 0; a0 < B; a0 += kBlock) {
            const int na = (B - a0 < kBlock) ? B - a0 : kBlock;
            if (reload) {
                __syncthreads();
                for (int i = threadIdx.x; i < na * NB; i += kThreads) cs[i] = Cp[(size_t)(a0 + i / NB) * ldc + b0 + i % NB];
                __syncthreads();
            }
            if (valid) {
                // the x_a[k] of the next 8 members are in flight while the multiply-adds of these 8 run (one load per member and lane)
                constexpr int U = 8;
                const double* xp = x + (size_t)a0 * n + k;
                double xc[U], xn[U];
#pragma unroll
                for (int u = 0; u < U; ++u) xc[u] = (u < na) ? xp[(size_t)u * n] : 0.0;
#pragma unroll 1
                for (int a = 0; a < na; a += U) {
#pragma unroll
                    for (int u = 0; u < U; ++u) xn[u] = (a + U + u < na) ? xp[(size_t)(a + U + u) * n] : 0.0;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (a + u < na) {
#pragma unroll
                            for (int j = 0; j < NB; ++j) acc[j] = __builtin_fma(cs[(a + u) * NB + j], xc[u], acc[j]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) xc[u] = xn[u];
                }
            }
        }
        if (valid) {
            double* o = out + (size_t)b0 * n + k;                             // (stepped, so that NB addresses are not kept over the tile loop)
            const int nout = B - b0;
            if (nout >= NB) {
#pragma unroll
                for (int j = 0; j < NB; ++j, o += n) *o = acc[j];
            } else {
#pragma unroll
                for (int j = 0; j < NB; ++j, o += n)
                    if (j < nout) *o = acc[j];
            }
        }
    }
}

bool misaligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }
// any overlap of two ranges of `len` doubles
bool overlap(const double* a, const double* b, size_t len) {
    const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b), bytes = len * sizeof(double);
    return ua < ub + bytes && ub < ua + bytes;
}

}  // namespace

double Context::block_scale() const {
    if (n_slabs() != 1 || cfg.world != 1) return 0.0;
    if (cfg.kind == SMO_KDYN) return (double)(vec_len / 3);
    if (cfg.kind == SMO_SH23) return (double)vec_len;
    return 0.0;
}

int Context::block_register() {
    if (!(block_scale() > 0.0)) return SMO_OK;
    const double vec_b = (double)cfg.batch * (double)vec_len * 8.0;
    bo.k_gram_xx = timing.add_class("block_gram(x,x)", vec_b);
    bo.k_gram_xy = timing.add_class("block_gram(x,y)", 2.0 * vec_b);
    bo.k_combine = timing.add_class("block_combine", 2.0 * vec_b);
    return SMO_OK;
}

int Context::block_check(const char* who) {
    if (!(block_scale() > 0.0) || bo.k_combine < 0) {
        set_error("%s: this context's inner product carries weights or its vectors are distributed (SHB23, POIS, slab and multi-device contexts); "
                  "the Gram matrix and the recombination serve KDYN on one GPU and SH23", who);
        return SMO_ERR_UNSUPPORTED;
    }
    if (cfg.batch > blockops::kMaxBatch) {
        set_error("%s: batch = %d (at most %d members)", who, cfg.batch, blockops::kMaxBatch);
        return SMO_ERR_UNSUPPORTED;
    }
    return SMO_OK;
}

int Context::gram_dev(const double* x, const double* y, double* out_host) {
    SMO_TRY(block_check("smo_gram_dev"));
    if (misaligned8(x) || misaligned8(y) || misaligned8(out_host)) {
        set_error("smo_gram_dev: pointers must be 8-byte aligned (x=%p y=%p out=%p)", (const void*)x, (const void*)y, (void*)out_host);
        return SMO_ERR_ARG;
    }
    const int B = cfg.batch;
    const GramPlan p = gram_plan(B, vec_len);
    const size_t need = (size_t)p.nwg * B * B;
    if (bo.partial_len < need) {
        if (bo.d_partial) SMO_TRY(pool.free_one(bo.d_partial));
        bo.d_partial = nullptr; bo.partial_len = 0;
        SMO_TRY(pool.alloc(&bo.d_partial, need));
        bo.partial_len = need;
    }
    if (!bo.d_out) SMO_TRY(pool.alloc(&bo.d_out, (size_t)B * B));
    const int sym = (x == y) ? 1 : 0;
    const dim3 grid(p.nwg, p.nblk, p.nblk);
    {
        ScopedTimer t(timing, sym ? bo.k_gram_xx : bo.k_gram_xy, stream, true);
#define SMO_BG(NT, KC) SMO_LAUNCH_T(t, (block_gram<NT, KC>), grid, dim3(kThreads), 0, stream, x, y, bo.d_partial, p, sym)
        if (p.kc == 512) SMO_BG(1, 512);
        else if (p.kc == 256) SMO_BG(1, 256);
        else if (p.kc == 128) SMO_BG(1, 128);
        else if (p.kc == 64) SMO_BG(2, 64);
        else if (p.nt == 3) SMO_BG(3, 32);
        else SMO_BG(4, 32);
#undef SMO_BG
    }
    SMO_HIP(hipGetLastError());
    SMO_LAUNCH(block_gram_finish, dim3((B * B + 7) / 8), dim3(kThreads), 0, stream, (const double*)bo.d_partial, bo.d_out, B, p.nwg,
                       block_scale(), sym);
    SMO_HIP(hipGetLastError());
    SMO_HIP(hipMemcpyAsync(out_host, bo.d_out, (size_t)B * B * sizeof(double), hipMemcpyDeviceToHost, stream));
    SMO_HIP(hipStreamSynchronize(stream));
    return SMO_OK;
}

int Context::combine_dev(const double* C_host, const double* x, double* out) {
    SMO_TRY(block_check("smo_combine_dev"));
    if (misaligned8(C_host) || misaligned8(x) || misaligned8(out)) {
        set_error("smo_combine_dev: pointers must be 8-byte aligned (C=%p x=%p out=%p)", (const void*)C_host, (const void*)x, (void*)out);
        return SMO_ERR_ARG;
    }
    const int B = cfg.batch;
    const size_t n = vec_len, total = (size_t)B * n;
    if (overlap(x, out, total)) {
        set_error("smo_combine_dev: out overlaps x (every output member reads every input member: the product is not done in place)");
        return SMO_ERR_ARG;
    }
    const int nb = combine_cols(B), ncb = (B + nb - 1) / nb, ldc = nb * ncb;
    bo.h_C.assign((size_t)B * ldc, 0.0);                                        // zero beyond column B: the padded outputs are computed, never stored
    for (int a = 0; a < B; ++a) std::copy(C_host + (size_t)a * B, C_host + (size_t)(a + 1) * B, bo.h_C.begin() + (size_t)a * ldc);
    if (!bo.d_C) SMO_TRY(pool.alloc(&bo.d_C, bo.h_C.size()));
    SMO_HIP(hipMemcpyAsync(bo.d_C, bo.h_C.data(), bo.h_C.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    const size_t ntiles = combine_wgs(n);
    const dim3 grid((unsigned)std::min<size_t>(ntiles, 2048), ncb);
    {
        ScopedTimer t(timing, bo.k_combine, stream, true);
#define SMO_BC(NB) SMO_LAUNCH_T(t, block_combine<NB>, grid, dim3(kThreads), 0, stream, x, (const double*)bo.d_C, out, B, n, ldc, ntiles)
        if (nb == 4) SMO_BC(4);
        else if (nb == 16) SMO_BC(16);
        else if (nb == 32) SMO_BC(32);
        else SMO_BC(64);
#undef SMO_BC
    }
    SMO_HIP(hipGetLastError());
    SMO_HIP(hipStreamSynchronize(stream));
    return SMO_OK;
}

// host vectors: staged through the context's device buffers like smo_inner
int Context::gram_host(const double* x, const double* y, double* out) {
    SMO_TRY(block_check("smo_gram"));
    if (misaligned8(x) || misaligned8(y) || misaligned8(out)) { set_error("smo_gram: pointers must be 8-byte aligned"); return SMO_ERR_ARG; }
    const size_t n = vec_len * (size_t)cfg.batch;
    for (int c = 0; c < 2; ++c)
        if (!stage_g[c]) SMO_TRY(pool.alloc(&stage_g[c], n));
    SMO_HIP(hipMemcpyAsync(stage_g[0], x, n * sizeof(double), hipMemcpyHostToDevice, stream));
    if (y != x) SMO_HIP(hipMemcpyAsync(stage_g[1], y, n * sizeof(double), hipMemcpyHostToDevice, stream));
    return gram_dev(stage_g[0], y == x ? stage_g[0] : stage_g[1], out);
}

int Context::combine_host(const double* C_host, const double* x, double* out) {
    SMO_TRY(block_check("smo_combine"));
    if (misaligned8(C_host) || misaligned8(x) || misaligned8(out)) { set_error("smo_combine: pointers must be 8-byte aligned"); return SMO_ERR_ARG; }
    const size_t n = vec_len * (size_t)cfg.batch;
    if (overlap(x, out, n)) { set_error("smo_combine: out overlaps x (the product is not done in place)"); return SMO_ERR_ARG; }
    for (int c = 0; c < 2; ++c)
        if (!stage_g[c]) SMO_TRY(pool.alloc(&stage_g[c], n));
    SMO_HIP(hipMemcpyAsync(stage_g[0], x, n * sizeof(double), hipMemcpyHostToDevice, stream));
    SMO_TRY(combine_dev(C_host, stage_g[0], stage_g[1]));
    SMO_HIP(hipMemcpyAsync(out, stage_g[1], n * sizeof(double), hipMemcpyDeviceToHost, stream));
    SMO_HIP(hipStreamSynchronize(stream));
    return SMO_OK;
}

}  // namespace smo
