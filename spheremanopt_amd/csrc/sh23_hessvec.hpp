// SH23 — Hessian-vector products of the discrete cost: the tangent sweep and the second-order adjoint sweep.
//
// Included by sh23.hip inside its unnamed namespace, behind pack_mode / unpack_mode / any_pack / any_unpack / zero_gap, sbdf1_step / compat and
// sh_n1 / sh_n2 / sh_src_q / sh_src_r, which the four
// kernels below share with the forward / adjoint pair.  Same shape as that pair: one workgroup per member runs the whole time loop, the
// per-mode state lives in registers (instantiated lengths) or in the LDS (any length), one 2 KB record per step goes to or comes from each
// HBM-resident stack, and the next step's records are fetched under the transforms.
//
//   tangent (forward in time, direction V):   d^_0 = F V;  for n = 0..N:  store d^_n;  (u, d) = F^-1 (u^_n, d^_n);  df += -2 dt mean(u d);
//                                             d^_{n+1} = (d^_n / dt + F[N'(u) d]) / A
//   second-order adjoint (backward):          q^ = -2 u^_N / A,  r^ = -2 d^_N / A;  for idx = N-1..0:  (u, d, q, r) = F^-1 (u^_idx, d^_idx, q^, r^);
//                                             q^ <- (q^ / dt + F[N'(u) q - 2 u]) / A;   r^ <- (r^ / dt + F[N'(u) r + N''(u) d q - 2 d]) / A
//                                             H V = F^-1[dt A r^],  grad f = F^-1[dt A q^]
// with N(u) = 1.8 u^2 - u^3, N'(u) = 3.6 u - 3 u^2, N''(u) = 3.6 - 6 u.
#pragma once

constexpr int TAN_THREADS = 128;     // two wavefronts: the two inverse transforms (u, d) side by side
constexpr int SOA_THREADS = 256;     // four wavefronts: one per inverse transform (q, r, u, d)
constexpr size_t SH_LDS_BYTES = 160 * 1024;       // LDS of one gfx950 workgroup

// Four transforms side by side take P, bufA, bufB of 4 NH elements each and the twiddles: 13 NH elements, 159 744 B at NH = 768.  Longer
// lengths run the inverse transforms as two rounds of two — (u, d) into a kept buffer K, then (q, r) — on 2 NH-element buffers: 9 NH
// elements, 147 456 B at NH = 1024.  The arithmetic per grid point and per mode is the same in both forms.
template <int NH> constexpr bool soa_wide() { return 13 * (size_t)NH * sizeof(cplx) <= SH_LDS_BYTES; }

template <int NH>
__global__ __launch_bounds__(TAN_THREADS) void sh23_tangent_kernel(const double* __restrict__ V, const cplx* __restrict__ stack, cplx* __restrict__ dstack,
                                                                   double* __restrict__ dJ, const double* __restrict__ A_g, const cplx* __restrict__ tw_g,
                                                                   const cplx* __restrict__ tw2_g, double dt, int n_iters, size_t a_stride,
                                                                   const int* __restrict__ Nh) {
    constexpr int NT = TAN_THREADS, NC = NH / 2, G = 2 * NH;
    constexpr int KPT = (NC + NT - 1) / NT;
    __shared__ cplx P[2 * NH], bufA[2 * NH], bufB[2 * NH], tw[NH];
    __shared__ double red[NT / 64];
    const int tid = threadIdx.x;
    const size_t prob = blockIdx.x;
    V += prob * G;
    stack += prob * (size_t)(n_iters + 1) * NC;                                  // (stride: the capacity cfg.n_iters)
    dstack += prob * (size_t)(n_iters + 1) * NC;
    if (Nh) n_iters = Nh[prob];                                                  // members with their own horizon (smo_set_horizons): this problem's loop bound
    A_g += prob * a_stride;                           // members with their own a: one table each (stride 0: the shared one)

    for (int i = tid; i < NH; i += NT) {
        tw[i] = tw_g[i];
        P[i] = mk(V[2 * i], V[2 * i + 1]);
    }
    cplx dh[KPT], w2[KPT], uf[KPT];
    double A[KPT];
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const int k = tid + i * NT;
        const bool ok = k < NC;
        w2[i] = ok ? tw2_g[k] : mk(1, 0);
        A[i] = ok ? A_g[k] : 1.0;
        dh[i] = mk(0, 0);
        uf[i] = ok ? stack[k] : mk(0, 0);             // u^_0
    }
    __syncthreads();

    auto ldP = [&](int b, int pos) { return P[b * NH + pos]; };
    auto stP = [&](int b, int pos, cplx v) { P[b * NH + pos] = v; };
    const double inv_dt = 1.0 / dt, inv_G = 1.0 / G;
    double acc = 0.0;

    for (int n = -1; n <= n_iters; ++n) {
        if (n >= 0) {
            fft_batch<NH, true>(bufA, bufB, tw, 2, NH, tid, NT, ldP, stP);        // P[0] = u_n, P[1] = d_n on the grid
            __syncthreads();
            for (int j = tid; j < NH; j += NT) {
                const cplx u = P[j], d = P[NH + j];
                acc += u.re * d.re + u.im * d.im;
                P[j] = mk(sh_n1(u.re) * d.re, sh_n1(u.im) * d.im);
            }
            if (n == n_iters) break;                  // d^_{N+1} is never used
            __syncthreads();
        }
        fft_batch<NH, false>(bufA, bufB, tw, 1, NH, tid, NT, ldP, stP);
        __syncthreads();
        // even/odd split + implicit solve + record + packing of both fields of the next step (same thread owns k and NH-k)
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const int k = tid + i * NT;
            if (k < NC) {
                cplx Nk = inv_G * unpack_mode<NH>(P, k, w2[i]);
                if (n < 0) dh[i] = Nk;                // d^_0 = F V
                else dh[i] = sbdf1_step(dh[i], Nk, inv_dt, A[i]);
                dstack[(size_t)(n + 1) * NC + k] = dh[i];
                pack_mode<NH>(P, k, uf[i], w2[i]);
                pack_mode<NH>(P + NH, k, dh[i], w2[i]);
            }
        }
        if (tid == 0) { P[NC] = mk(0, 0); P[NH + NC] = mk(0, 0); }
        if (n + 2 <= n_iters) {                       // prefetch the next forward record under the transforms
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                const int k = tid + i * NT;
                if (k < NC) uf[i] = stack[(size_t)(n + 2) * NC + k];
            }
        }
        __syncthreads();
    }
    // df = -2 dt sum_n mean(u_n d_n)
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) dJ[prob] = -(2.0 * dt * inv_G) * (red[0] + red[1]);
}

template <int NH>
__global__ __launch_bounds__(SOA_THREADS) void sh23_soa_kernel(const cplx* __restrict__ stack, const cplx* __restrict__ dstack, double* __restrict__ HV,
                                                               double* __restrict__ grad, const double* __restrict__ A_g, const cplx* __restrict__ tw_g,
                                                               const cplx* __restrict__ tw2_g, double dt, int n_iters, size_t a_stride,
                                                               const int* __restrict__ Nh) {
    constexpr bool WIDE = soa_wide<NH>();
    constexpr int NT = SOA_THREADS, NC = NH / 2, G = 2 * NH, NB = WIDE ? 4 : 2;
    constexpr int KPT = (NC + NT - 1) / NT;
    __shared__ cplx lds[(3 * NB + 1 + (WIDE ? 0 : 2)) * NH];
    cplx* const P = lds;                              // [0] = q, [1] = r (WIDE: [2] = u, [3] = d)
    cplx* const bufA = P + NB * NH;
    cplx* const bufB = bufA + NB * NH;
    cplx* const tw = bufB + NB * NH;
    cplx* const K = WIDE ? P + 2 * NH : tw + NH;      // [0] = u, [1] = d on the grid
    const int tid = threadIdx.x;
    const size_t prob = blockIdx.x;
    stack += prob * (size_t)(n_iters + 1) * NC;                                  // (stride: the capacity cfg.n_iters)
    dstack += prob * (size_t)(n_iters + 1) * NC;
    if (Nh) n_iters = Nh[prob];                                                  // members with their own horizon (smo_set_horizons): this problem's loop bound
    HV += prob * G;
    if (grad) grad += prob * G;
    A_g += prob * a_stride;                           // members with their own a: one table each (stride 0: the shared one)

    for (int i = tid; i < NH; i += NT) tw[i] = tw_g[i];
    cplx qh[KPT], rh[KPT], w2[KPT], uf[KPT], df[KPT];
    double A[KPT];
    int idx = n_iters - 1;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const int k = tid + i * NT;
        const bool ok = k < NC;
        w2[i] = ok ? tw2_g[k] : mk(1, 0);
        A[i] = ok ? A_g[k] : 1.0;
        qh[i] = rh[i] = mk(0, 0);
        if (ok) {                                     // compatibility conditions  q^ = -2 u^_N / A,  r^ = -2 d^_N / A
            const cplx uN = stack[(size_t)n_iters * NC + k], dN = dstack[(size_t)n_iters * NC + k];
            qh[i] = mk(-2.0 * uN.re / A[i], -2.0 * uN.im / A[i]);
            rh[i] = mk(-2.0 * dN.re / A[i], -2.0 * dN.im / A[i]);
        }
        uf[i] = ok ? stack[(size_t)idx * NC + k] : mk(0, 0);
        df[i] = ok ? dstack[(size_t)idx * NC + k] : mk(0, 0);
    }
    const double inv_dt = 1.0 / dt, inv_G = 1.0 / G;
    auto ldP = [&](int b, int pos) { return P[b * NH + pos]; };
    auto stP = [&](int b, int pos, cplx v) { P[b * NH + pos] = v; };

    for (int it = 0; it < n_iters; ++it) {
        // (u, d) of this step, packed where their round reads them: behind (q, r) in P, or in P itself for a round of their own
        cplx* const PU = WIDE ? P + 2 * NH : P;
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const int k = tid + i * NT;
            if (k < NC) {
                pack_mode<NH>(PU, k, uf[i], w2[i]);
                pack_mode<NH>(PU + NH, k, df[i], w2[i]);
                if (WIDE) {
                    pack_mode<NH>(P, k, qh[i], w2[i]);
                    pack_mode<NH>(P + NH, k, rh[i], w2[i]);
                }
            }
        }
        if (tid < NB) P[tid * NH + NC] = mk(0, 0);
        --idx;
        if (idx >= 0) {                               // prefetch the next two records under the transforms
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                const int k = tid + i * NT;
                if (k < NC) { uf[i] = stack[(size_t)idx * NC + k]; df[i] = dstack[(size_t)idx * NC + k]; }
            }
        }
        __syncthreads();
        if (WIDE) {
            fft_batch<NH, true>(bufA, bufB, tw, 4, NH, tid, NT, ldP, stP);    // P[0..3] = q, r, u, d on the grid
            __syncthreads();
        } else {
            fft_batch<NH, true>(bufA, bufB, tw, 2, NH, tid, NT, ldP, [&](int b, int pos, cplx v) { K[b * NH + pos] = v; });
            __syncthreads();
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                const int k = tid + i * NT;
                if (k < NC) {
                    pack_mode<NH>(P, k, qh[i], w2[i]);
                    pack_mode<NH>(P + NH, k, rh[i], w2[i]);
                }
            }
            if (tid < 2) P[tid * NH + NC] = mk(0, 0);
            __syncthreads();
            fft_batch<NH, true>(bufA, bufB, tw, 2, NH, tid, NT, ldP, stP);    // P[0..1] = q, r on the grid
            __syncthreads();
        }
        for (int n = tid; n < NH; n += NT) {
            const cplx u = K[n], d = K[NH + n], q = P[n], r = P[NH + n];
            P[n] = mk(sh_src_q(u.re, q.re), sh_src_q(u.im, q.im));
            P[NH + n] = mk(sh_src_r(u.re, d.re, q.re, r.re), sh_src_r(u.im, d.im, q.im, r.im));
        }
        __syncthreads();
        fft_batch<NH, false>(bufA, bufB, tw, 2, NH, tid, NT, ldP, stP);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const int k = tid + i * NT;
            if (k < NC) {
                const cplx Hq = inv_G * unpack_mode<NH>(P, k, w2[i]);
                const cplx Hr = inv_G * unpack_mode<NH>(P + NH, k, w2[i]);
                qh[i] = mk((qh[i].re * inv_dt + Hq.re) / A[i], (qh[i].im * inv_dt + Hq.im) / A[i]);
                rh[i] = mk((rh[i].re * inv_dt + Hr.re) / A[i], (rh[i].im * inv_dt + Hr.im) / A[i]);
            }
        }
        __syncthreads();
    }
    // on the scale-2 grid:  H V = F^-1[dt (1/dt + L) r^]  and, when asked for,  grad f = F^-1[dt (1/dt + L) q^]
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const int k = tid + i * NT;
        if (k < NC) {
            const double s = dt * A[i];
            pack_mode<NH>(P, k, mk(s * rh[i].re, s * rh[i].im), w2[i]);
            pack_mode<NH>(P + NH, k, mk(s * qh[i].re, s * qh[i].im), w2[i]);
        }
    }
    if (tid < 2) P[tid * NH + NC] = mk(0, 0);
    __syncthreads();
    fft_batch<NH, true>(bufA, bufB, tw, 2, NH, tid, NT, ldP, [&](int b, int pos, cplx v) {
        double* out = b ? grad : HV;
        if (out) { out[2 * pos] = v.re; out[2 * pos + 1] = v.im; }
    });
}

// ---------------------------------------------------------------------------------------------------------
// Any Npts: the same two sweeps with NH a run-time value, the per-mode state in the LDS (see sh23_forward_any / sh23_adjoint_any).
// ---------------------------------------------------------------------------------------------------------
inline size_t tangent_any_lds(int NH, int NC) { return (size_t)(5 * NH + NC) * sizeof(cplx); }                 // P, T: 2 NH each; twiddles; d^
// wide: two buffers of four transforms; else three buffers of two (u, d stay in one of them while q, r are transformed)
inline size_t soa_any_lds(int NH, int NC, bool wide) { return (size_t)((wide ? 9 : 7) * NH + 2 * NC) * sizeof(cplx); }

__global__ __launch_bounds__(ANY_THREADS) void sh23_tangent_any(const double* __restrict__ V, const cplx* __restrict__ stack, cplx* __restrict__ dstack,
                                                                double* __restrict__ dJ, const double* __restrict__ A_g, const cplx* __restrict__ tw_g,
                                                                const cplx* __restrict__ tw2_g, double dt, int n_iters, AnyPlan pl, int NC, size_t a_stride,
                                                                const int* __restrict__ Nh) {
    extern __shared__ cplx sh_lds[];
    const int NT = blockDim.x;                                                   // 64 .. ANY_THREADS, a multiple of 64
    const int NH = pl.L, G = 2 * NH, tid = threadIdx.x;
    cplx *P = sh_lds, *T = sh_lds + 2 * NH, *tws = sh_lds + 4 * NH, *dh = sh_lds + 5 * NH;              // P / T: two transforms side by side (u, d)
    any_load_tw(tws, tw_g, NH, tid, NT);
    __shared__ double red[ANY_THREADS / 64];
    const size_t prob = blockIdx.x;
    V += prob * G;
    stack += prob * (size_t)(n_iters + 1) * NC;                                  // (stride: the capacity cfg.n_iters)
    dstack += prob * (size_t)(n_iters + 1) * NC;
    if (Nh) n_iters = Nh[prob];                                                  // members with their own horizon (smo_set_horizons): this problem's loop bound
    A_g += prob * a_stride;                                                      // members with their own a (stride 0: the shared table)
    for (int i = tid; i < NH; i += NT) P[i] = mk(V[2 * i], V[2 * i + 1]);
    for (int k = tid; k < NC; k += NT) dh[k] = mk(0, 0);
    __syncthreads();
    const double inv_dt = 1.0 / dt, inv_G = 1.0 / G;
    double acc = 0.0;
    for (int n = -1; n <= n_iters; ++n) {
        cplx* src = P;                                                           // what the forward transform reads: V, then N'(u) d
        if (n >= 0) {
            const cplx* R = any_fft<true>(P, T, tws, pl, 2, tid, NT);          // R[0..NH) = u_n, R[NH..2NH) = d_n on the grid
            src = (R == P) ? T : P;
            for (int i = tid; i < NH; i += NT) {
                const cplx u = R[i], d = R[NH + i];
                acc += u.re * d.re + u.im * d.im;
                src[i] = mk(sh_n1(u.re) * d.re, sh_n1(u.im) * d.im);
            }
            if (n == n_iters) break;
            __syncthreads();
        }
        const cplx* H = any_fft<false>(src, (src == P) ? T : P, tws, pl, 1, tid, NT);
        for (int k = tid; k < NC; k += NT) {                                    // the same thread owns k and NH - k: in place is safe
            const cplx w = tw2_g[k];
            const cplx Nk = inv_G * any_unpack(H, NH, k, w);
            const cplx d = (n < 0) ? Nk : sbdf1_step(dh[k], Nk, inv_dt, A_g[k]);
            dh[k] = d;
            dstack[(size_t)(n + 1) * NC + k] = d;
            any_pack(P, NH, k, stack[(size_t)(n + 1) * NC + k], w);
            any_pack(P + NH, NH, k, d, w);
        }
        zero_gap(P, NH, NC, tid, NT);
        zero_gap(P + NH, NH, NC, tid, NT);
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) { double s = 0.0; for (int i = 0; i < NT / 64; ++i) s += red[i]; dJ[prob] = -(2.0 * dt * inv_G) * s; }
}

__global__ __launch_bounds__(ANY_THREADS) void sh23_soa_any(const cplx* __restrict__ stack, const cplx* __restrict__ dstack, double* __restrict__ HV,
                                                            double* __restrict__ grad, const double* __restrict__ A_g, const cplx* __restrict__ tw_g,
                                                            const cplx* __restrict__ tw2_g, double dt, int n_iters, AnyPlan pl, int NC, int wide,
                                                            size_t a_stride, const int* __restrict__ Nh) {
    extern __shared__ cplx sh_lds[];
    const int NT = blockDim.x;
    const int NH = pl.L, G = 2 * NH, tid = threadIdx.x;
    const int NB = wide ? 4 : 2;
    cplx *B0 = sh_lds, *B1 = B0 + NB * NH, *B2 = B1 + NB * NH;                  // (B2: the third buffer of the two-round form only)
    cplx *tws = sh_lds + (wide ? 8 : 6) * NH, *qh = tws + NH, *rh = qh + NC;
    any_load_tw(tws, tw_g, NH, tid, NT);
    const size_t prob = blockIdx.x;
    stack += prob * (size_t)(n_iters + 1) * NC;                                  // (stride: the capacity cfg.n_iters)
    dstack += prob * (size_t)(n_iters + 1) * NC;
    if (Nh) n_iters = Nh[prob];                                                  // members with their own horizon (smo_set_horizons): this problem's loop bound
    HV += prob * G;
    if (grad) grad += prob * G;
    A_g += prob * a_stride;                                                      // members with their own a (stride 0: the shared table)
    for (int k = tid; k < NC; k += NT) {                                        // (qh[k], rh[k] are read and written by the same thread only)
        const cplx uN = stack[(size_t)n_iters * NC + k], dN = dstack[(size_t)n_iters * NC + k];
        qh[k] = mk(-2.0 * uN.re / A_g[k], -2.0 * uN.im / A_g[k]);
        rh[k] = mk(-2.0 * dN.re / A_g[k], -2.0 * dN.im / A_g[k]);
    }
    const double inv_dt = 1.0 / dt, inv_G = 1.0 / G;
    for (int idx = n_iters - 1; idx >= 0; --idx) {
        cplx* const PU = wide ? B0 + 2 * NH : B0;
        for (int k = tid; k < NC; k += NT) {
            const cplx w = tw2_g[k];
            any_pack(PU, NH, k, stack[(size_t)idx * NC + k], w);
            any_pack(PU + NH, NH, k, dstack[(size_t)idx * NC + k], w);
            if (wide) { any_pack(B0, NH, k, qh[k], w); any_pack(B0 + NH, NH, k, rh[k], w); }
        }
        for (int b = 0; b < NB; ++b) zero_gap(B0 + b * NH, NH, NC, tid, NT);
        __syncthreads();
        cplx *Q, *U, *F;                                                         // (q, r) and (u, d) on the grid; the free buffer
        if (wide) {
            Q = any_fft<true>(B0, B1, tws, pl, 4, tid, NT);
            U = Q + 2 * NH;
            F = (Q == B0) ? B1 : B0;
        } else {
            U = any_fft<true>(B0, B1, tws, pl, 2, tid, NT);
            cplx* X = (U == B0) ? B1 : B0;
            for (int k = tid; k < NC; k += NT) {
                const cplx w = tw2_g[k];
                any_pack(X, NH, k, qh[k], w);
                any_pack(X + NH, NH, k, rh[k], w);
            }
            zero_gap(X, NH, NC, tid, NT);
            zero_gap(X + NH, NH, NC, tid, NT);
            __syncthreads();
            Q = any_fft<true>(X, B2, tws, pl, 2, tid, NT);
            F = (Q == X) ? B2 : X;
        }
        for (int i = tid; i < NH; i += NT) {
            const cplx u = U[i], d = U[NH + i], q = Q[i], r = Q[NH + i];
            F[i] = mk(sh_src_q(u.re, q.re), sh_src_q(u.im, q.im));
            F[NH + i] = mk(sh_src_r(u.re, d.re, q.re, r.re), sh_src_r(u.im, d.im, q.im, r.im));
        }
        __syncthreads();
        const cplx* H = any_fft<false>(F, Q, tws, pl, 2, tid, NT);
        for (int k = tid; k < NC; k += NT) {
            const cplx w = tw2_g[k];
            const cplx Hq = inv_G * any_unpack(H, NH, k, w), Hr = inv_G * any_unpack(H + NH, NH, k, w);
            qh[k] = mk((qh[k].re * inv_dt + Hq.re) / A_g[k], (qh[k].im * inv_dt + Hq.im) / A_g[k]);
            rh[k] = mk((rh[k].re * inv_dt + Hr.re) / A_g[k], (rh[k].im * inv_dt + Hr.im) / A_g[k]);
        }
        __syncthreads();
    }
    // on the scale-2 grid:  H V = F^-1[dt (1/dt + L) r^]  and, when asked for,  grad f = F^-1[dt (1/dt + L) q^]
    for (int k = tid; k < NC; k += NT) {
        const double s = dt * A_g[k];
        const cplx w = tw2_g[k];
        any_pack(B0, NH, k, mk(s * rh[k].re, s * rh[k].im), w);
        any_pack(B0 + NH, NH, k, mk(s * qh[k].re, s * qh[k].im), w);
    }
    zero_gap(B0, NH, NC, tid, NT);
    zero_gap(B0 + NH, NH, NC, tid, NT);
    __syncthreads();
    const cplx* R = any_fft<true>(B0, B1, tws, pl, 2, tid, NT);
    for (int i = tid; i < NH; i += NT) {
        HV[2 * i] = R[i].re; HV[2 * i + 1] = R[i].im;
        if (grad) { grad[2 * i] = R[NH + i].re; grad[2 * i + 1] = R[NH + i].im; }
    }
}
