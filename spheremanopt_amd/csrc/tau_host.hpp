// Chebyshev-tau operators of the SHB23 and the Poiseuille paths (host side: Chebyshev pieces, assembly of the tau systems, one LU).
//
// Every step of SHB23 and of both Poiseuille formulations applies an operator S = (rows of) A^-1 B, A the tau system of the step's
// boundary-value problem and B the T -> U conversion of its right-hand sides.  With unknowns and equations interleaved by Chebyshev mode
// A is banded apart from a few dense boundary rows, and lu_solve() is a partial-pivot LU that knows it.  Each operator is built in two
// pieces, the assembly of (A, B) and the solve, so that a test can hand the same system to a second solver.
//
// Everything here is host code without HIP types: tests/c/tau_host_test.cpp drives it on the CPU (structured LU == plain LU byte for
// byte, Pre * D == PD exactly, Tf Ti == I to rounding, every operator against the NumPy oracle's builder).
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <vector>

#include "hodlr.hpp"

namespace smo {
namespace tau {

using cd = std::complex<double>;

// Solve A X = B (A n x n with structural zeros, B n x m) in place by LU with partial pivoting.  The tau systems are banded (unknowns
// and equations interleaved by Chebyshev mode) apart from a few dense boundary rows kept at the bottom (rows >= nb): column k can only
// be non-zero in the `win` rows below the diagonal and in the dense rows, so those are the pivot candidates and the rows to
// eliminate; a per-row "last non-zero column" bound keeps the row operations inside the (growing) band.  nb = win = n: every row at or
// below k is searched and eliminated (SHB23, whose boundary rows sit inside the last block).
// Returns -1, or the column at which no pivot was found.
template <class T> int lu_solve(int n, int nb, int win, std::vector<T>& A, int m, std::vector<T>& B) {
    auto at = [&](int r, int c) -> T& { return A[(size_t)r * n + c]; };
    std::vector<int> hi(n, 0);
    for (int r = 0; r < n; ++r)
        for (int c = n - 1; c >= 0; --c) if (at(r, c) != T(0)) { hi[r] = c; break; }
    for (int k = 0; k < n; ++k) {
        const int wend = std::min(n, k + win), dense0 = std::max(wend, nb);
        int p = -1; double best = 0.0;
        auto consider = [&](int r) { const double v = std::abs(at(r, k)); if (v > best) { best = v; p = r; } };
        for (int r = k; r < wend; ++r) consider(r);
        for (int r = dense0; r < n; ++r) consider(r);
        if (p < 0) return k;
        if (p != k) {
            std::swap_ranges(&at(k, 0), &at(k, 0) + n, &at(p, 0));
            std::swap_ranges(&B[(size_t)k * m], &B[(size_t)k * m] + m, &B[(size_t)p * m]);
            std::swap(hi[k], hi[p]);
        }
        const T piv = at(k, k);
        const int hk = hi[k];
        auto elim = [&](int r) {
            const T f = at(r, k);
            if (f == T(0)) return;
            const T l = f / piv;
            at(r, k) = 0;
            T* ar = &at(r, 0); const T* ak = &at(k, 0);
            for (int c = k + 1; c <= hk; ++c) ar[c] -= l * ak[c];
            T* br = &B[(size_t)r * m]; const T* bk = &B[(size_t)k * m];
            for (int j = 0; j < m; ++j) br[j] -= l * bk[j];
            hi[r] = std::max(hi[r], hk);
        };
        for (int r = k + 1; r < wend; ++r) elim(r);
        for (int r = std::max(dense0, k + 1); r < n; ++r) elim(r);
    }
    for (int k = n - 1; k >= 0; --k) {
        T* bk = &B[(size_t)k * m];
        for (int c = k + 1; c <= hi[k]; ++c) {
            const T u = at(k, c);
            if (u == T(0)) continue;
            const T* bc = &B[(size_t)c * m];
            for (int j = 0; j < m; ++j) bk[j] -= u * bc[j];
        }
        const T inv = 1.0 / at(k, k);
        for (int j = 0; j < m; ++j) bk[j] *= inv;
    }
    return -1;
}

// ---------------------------------------------------------------------------------------------------------
// SHB23: the 4N x 4N system of a step, and S (N x N): rhs of the first equation -> u
// ---------------------------------------------------------------------------------------------------------
// Unknown / equation numbering interleaved by Chebyshev mode (index 4*n + v) so the system is banded apart from the four
// boundary rows.  Equations (T -> U conversion "Pre" applied, last row of each block replaced by a boundary row):
//   e0: Pre[(1/dt + 1 - a) u + 2 uzz + D uzzz] = Pre rhs      bc: left(uz)   = 0
//   e1: Pre[uz   - D u  ] = 0                                  bc: left(uzzz) = 0
//   e2: Pre[uzz  - D uz ] = 0                                  bc: right(u)   = 0
//   e3: Pre[uzzz - D uzz] = 0                                  bc: right(uzz) = 0
// Pre[n][n] = 1 (n=0) | 1/2, Pre[n][n+2] = -1/2;  (Pre D)[n][n+1] = (n+1)/stretch  (d/dx T_n = n U_{n-1}).
inline void shb_assemble(int N, double dt, double a, double z0, double z1, std::vector<double>& A, std::vector<double>& B) {
    const int n4 = 4 * N;
    const double stretch = 0.5 * (z1 - z0), c0 = 1.0 / dt + 1.0 - a;
    A.assign((size_t)n4 * n4, 0.0); B.assign((size_t)n4 * N, 0.0);
    auto at = [&](int r, int c) -> double& { return A[(size_t)r * n4 + c]; };
    auto pre_row = [&](int n, auto&& f) {            // f(col_mode, weight) over the non-zeros of row n of Pre
        f(n, n == 0 ? 1.0 : 0.5);
        if (n + 2 < N) f(n + 2, -0.5);
    };
    for (int n = 0; n < N - 1; ++n) {                 // rows 0..N-2 of every block; row N-1 holds the boundary condition
        pre_row(n, [&](int j, double w) {
            at(4 * n + 0, 4 * j + 0) += w * c0;  at(4 * n + 0, 4 * j + 2) += w * 2.0;
            at(4 * n + 1, 4 * j + 1) += w;       at(4 * n + 2, 4 * j + 2) += w;     at(4 * n + 3, 4 * j + 3) += w;
            B[(size_t)(4 * n + 0) * N + j] += w;                                      // Pre * rhs
        });
        const double d = (n + 1) / stretch;            // (Pre D)[n][n+1]
        at(4 * n + 0, 4 * (n + 1) + 3) += d;
        at(4 * n + 1, 4 * (n + 1) + 0) -= d;
        at(4 * n + 2, 4 * (n + 1) + 1) -= d;
        at(4 * n + 3, 4 * (n + 1) + 2) -= d;
    }
    const int bc_var[4] = {1, 3, 0, 2};
    const bool bc_left[4] = {true, true, false, false};
    for (int e = 0; e < 4; ++e)
        for (int j = 0; j < N; ++j) at(4 * (N - 1) + e, 4 * j + bc_var[e]) = (bc_left[e] && (j & 1)) ? -1.0 : 1.0;
}
// returns lu_solve's: -1, or the singular column
inline int shb_tau_operator(int N, double dt, double a, double z0, double z1, std::vector<double>& S) {
    std::vector<double> A, B;
    shb_assemble(N, dt, a, z0, z1, A, B);
    const int col = lu_solve(4 * N, 4 * N, 4 * N, A, N, B);
    if (col >= 0) return col;
    S.assign((size_t)N * N, 0.0);
    for (int n = 0; n < N; ++n) std::copy(&B[(size_t)(4 * n) * N], &B[(size_t)(4 * n) * N] + N, &S[(size_t)n * N]);
    return -1;
}

// ---------------------------------------------------------------------------------------------------------
// Poiseuille: Chebyshev pieces and the tau systems
// ---------------------------------------------------------------------------------------------------------
struct Cheb {
    int N;
    std::vector<double> Pre, D, PD, M1, M2, integ;          // dense N x N (row-major); PD = Pre * D
    explicit Cheb(int n) : N(n), Pre((size_t)n * n, 0.0), D((size_t)n * n, 0.0), PD((size_t)n * n, 0.0), M1((size_t)n * n, 0.0),
                           M2((size_t)n * n, 0.0), integ(n, 0.0) {
        for (int i = 0; i < N; ++i) {
            Pre[(size_t)i * N + i] = i == 0 ? 1.0 : 0.5;
            if (i + 2 < N) Pre[(size_t)i * N + i + 2] = -0.5;
            for (int j = i + 1; j < N; ++j) D[(size_t)i * N + j] = ((j - i) & 1) ? (i == 0 ? 1.0 : 2.0) * j : 0.0;
            integ[i] = (i & 1) ? 0.0 : 2.0 / (1.0 - (double)i * i);
        }
        for (int i = 0; i + 1 < N; ++i) PD[(size_t)i * N + i + 1] = i + 1;            // d/dz T_n = n U_{n-1}
        auto mult = [&](std::vector<double>& M, int j, double fj) {                    // T_j T_m = (T_{m+j} + T_{|m-j|}) / 2
            for (int m = 0; m < N; ++m) {
                if (m + j < N) M[(size_t)(m + j) * N + m] += 0.5 * fj;
                M[(size_t)std::abs(m - j) * N + m] += 0.5 * fj;
            }
        };
        mult(M1, 0, 0.5); mult(M1, 2, -0.5);                                           // 1 - z^2
        mult(M2, 1, -2.0);                                                             // -2 z
    }
    double pre_times(const std::vector<double>& M, int r, int c) const {              // (Pre * M)[r][c]
        double s = (r == 0 ? 1.0 : 0.5) * M[(size_t)r * N + c];
        if (r + 2 < N) s -= 0.5 * M[(size_t)(r + 2) * N + c];
        return s;
    }
};

// S_n (6N x 3N) of the momentum / density LBVP (POIS:818-841) for native wavenumber n (k = n * k1).
// Unknown index 7*mode + var (var: u v rho uz vz rhoz p) [+ Fb at the end for n = 0]; rows: for mode m < N-1 the seven equations
// (three tau-reduced evolution equations, continuity, three tau-reduced derivative definitions), then continuity of mode N-1, the
// six boundary / gauge rows [and integ(rho) = 0 for n = 0].
// adjoint = the operator of the script's adjoint IVP (POIS:1217-1252): advection by -U, Ri*w coupled into the density equation and
// Uz*u into the w equation (instead of Ri*rho into w and Uz*w into u).
inline int solve_unknowns(int N, int n) { return 7 * N + (n == 0 ? 1 : 0); }
constexpr int SOLVE_WIN = 7 * 6;                             // pivot window of the system below: six modes of seven rows
inline void assemble_solve_system(const Cheb& ch, int n, double k, double a0, double Re, double Pe, double Ri, bool adjoint, std::vector<cd>& A,
                                  std::vector<cd>& B) {
    const int N = ch.N, nv = solve_unknowns(N, n), nb = 7 * (N - 1);
    A.assign((size_t)nv * nv, cd(0)); B.assign((size_t)nv * 3 * N, cd(0));
    auto at = [&](int r, int c) -> cd& { return A[(size_t)r * nv + c]; };
    enum { U = 0, V = 1, R = 2, UZ = 3, VZ = 4, RZ = 5, P = 6 };
    const cd ik(0.0, k), adv(0.0, adjoint ? -k : k);
    for (int m = 0; m < N - 1; ++m) {
        const int r0 = 7 * m;
        for (int c = std::max(0, m - 2); c < std::min(N, m + 5); ++c) {
            const double pre = ch.Pre[(size_t)m * N + c], pm1 = ch.pre_times(ch.M1, m, c), pm2 = ch.pre_times(ch.M2, m, c),
                         pd = ch.PD[(size_t)m * N + c];
            at(r0 + 0, 7 * c + U) += (a0 + k * k / Re) * pre + adv * pm1;  at(r0 + 0, 7 * c + UZ) += -pd / Re;
            at(r0 + 0, 7 * c + P) += ik * pre;
            at(r0 + 1, 7 * c + V) += (a0 + k * k / Re) * pre + adv * pm1;  at(r0 + 1, 7 * c + VZ) += -pd / Re;
            at(r0 + 1, 7 * c + P) += pd;
            at(r0 + 2, 7 * c + R) += (a0 + k * k / Pe) * pre + adv * pm1;  at(r0 + 2, 7 * c + RZ) += -pd / Pe;
            if (!adjoint) { at(r0 + 0, 7 * c + V) += pm2;  at(r0 + 1, 7 * c + R) += Ri * pre; }
            else          { at(r0 + 1, 7 * c + U) += pm2;  at(r0 + 2, 7 * c + V) += Ri * pre; }
            at(r0 + 4, 7 * c + UZ) += pre;  at(r0 + 4, 7 * c + U) += -pd;
            at(r0 + 5, 7 * c + VZ) += pre;  at(r0 + 5, 7 * c + V) += -pd;
            at(r0 + 6, 7 * c + RZ) += pre;  at(r0 + 6, 7 * c + R) += -pd;
            for (int e = 0; e < 3; ++e) B[(size_t)(r0 + e) * 3 * N + e * N + c] = pre;
        }
        if (n == 0) at(r0 + 2, 7 * N) += ch.Pre[(size_t)m * N + 0];                   // + Fb (constant = its T0 coefficient)
        at(r0 + 3, 7 * m + U) += ik;  at(r0 + 3, 7 * m + VZ) += 1.0;                   // dx(u) + vz = 0
    }
    int row = nb;
    at(row, 7 * (N - 1) + U) += ik;  at(row, 7 * (N - 1) + VZ) += 1.0;  ++row;
    auto functional = [&](int var, int kind) {                                         // 0 left, 1 right, 2 integ
        for (int j = 0; j < N; ++j) at(row, 7 * j + var) = kind == 0 ? ((j & 1) ? -1.0 : 1.0) : (kind == 1 ? 1.0 : ch.integ[j]);
        ++row;
    };
    functional(U, 0); functional(V, 0); functional(U, 1);
    if (n != 0) functional(V, 1); else functional(P, 2);
    functional(RZ, 0); functional(RZ, 1);
    if (n == 0) functional(R, 2);
}
// returns lu_solve's: -1, or the singular column (of solve_unknowns(N, n))
inline int build_solve_map(const Cheb& ch, int n, double k, double a0, double Re, double Pe, double Ri, std::vector<cd>& S, bool adjoint = false) {
    const int N = ch.N;
    std::vector<cd> A, B;
    assemble_solve_system(ch, n, k, a0, Re, Pe, Ri, adjoint, A, B);
    const int col = lu_solve(solve_unknowns(N, n), 7 * (N - 1), SOLVE_WIN, A, 3 * N, B);
    if (col >= 0) return col;
    S.assign((size_t)6 * N * 3 * N, cd(0));
    for (int var = 0; var < 6; ++var)
        for (int j = 0; j < N; ++j) std::copy(&B[(size_t)(7 * j + var) * 3 * N], &B[(size_t)(7 * j + var) * 3 * N] + 3 * N, &S[((size_t)var * N + j) * 3 * N]);
    return -1;
}
// S^MN_n (2N x N): rho -> (psi, psiz),  dx dx psi + dz psiz + F = rho,  psiz = dz psi,  psiz(+-1) = 0,  integ psi = 0 at n = 0
inline int mixnorm_unknowns(int N, int n) { return 2 * N + (n == 0 ? 1 : 0); }
constexpr int MIXNORM_WIN = 2 * 4;
inline void assemble_mixnorm_system(const Cheb& ch, int n, double k, std::vector<cd>& A, std::vector<cd>& B) {
    const int N = ch.N, nv = mixnorm_unknowns(N, n), nb = 2 * (N - 1);
    A.assign((size_t)nv * nv, cd(0)); B.assign((size_t)nv * N, cd(0));
    auto at = [&](int r, int c) -> cd& { return A[(size_t)r * nv + c]; };
    for (int m = 0; m < N - 1; ++m) {
        for (int c = m; c < std::min(N, m + 3); ++c) {
            const double pre = ch.Pre[(size_t)m * N + c], pd = ch.PD[(size_t)m * N + c];
            at(2 * m, 2 * c) += -k * k * pre;  at(2 * m, 2 * c + 1) += pd;
            at(2 * m + 1, 2 * c + 1) += pre;   at(2 * m + 1, 2 * c) += -pd;
            B[(size_t)(2 * m) * N + c] = pre;
        }
        if (n == 0) at(2 * m, 2 * N) += ch.Pre[(size_t)m * N + 0];
    }
    for (int j = 0; j < N; ++j) { at(nb, 2 * j + 1) = (j & 1) ? -1.0 : 1.0; at(nb + 1, 2 * j + 1) = 1.0; }
    if (n == 0) for (int j = 0; j < N; ++j) at(nb + 2, 2 * j) = ch.integ[j];
}
inline int build_mixnorm_map(const Cheb& ch, int n, double k, std::vector<cd>& S) {
    const int N = ch.N;
    std::vector<cd> A, B;
    assemble_mixnorm_system(ch, n, k, A, B);
    const int col = lu_solve(mixnorm_unknowns(N, n), 2 * (N - 1), MIXNORM_WIN, A, N, B);
    if (col >= 0) return col;
    S.assign((size_t)2 * N * N, cd(0));
    for (int var = 0; var < 2; ++var)
        for (int j = 0; j < N; ++j) std::copy(&B[(size_t)(2 * j + var) * N], &B[(size_t)(2 * j + var) * N] + N, &S[((size_t)var * N + j) * N]);
    return -1;
}

// ---------------------------------------------------------------------------------------------------------
// host pieces of init() that the two Poiseuille formulations build the same way (same expressions, same accumulation order)
// ---------------------------------------------------------------------------------------------------------
inline std::vector<double> transposed(const std::vector<double>& M, int rows, int cols) {          // M rows x cols (row-major) -> cols x rows
    std::vector<double> t((size_t)rows * cols);
    for (int i = 0; i < rows; ++i) for (int j = 0; j < cols; ++j) t[(size_t)j * rows + i] = M[(size_t)i * cols + j];
    return t;
}
// the Gauss grid z of G points and the Chebyshev pair between a grid line and its first N T coefficients: Tf (N x G) grid -> coefficients
// (transform, POIS:44-51), Ti (G x N) back (transformInverse, POIS:67-76).  G = N in the Discrete formulation, 3N/2 in the Continuous one
inline void cheb_pair(int N, int G, std::vector<double>& Tf, std::vector<double>& Ti, std::vector<double>& z) {
    Tf.assign((size_t)N * G, 0.0); Ti.assign((size_t)G * N, 0.0); z.assign(G, 0.0);
    for (int i = 0; i < G; ++i) z[i] = -std::cos(M_PI * (i + 0.5) / G);
    // cos(pi j (2i + 1) / (2G)): the argument reaches j pi, and in double its rounding alone moved the entries by up to 3.4 N ulp (1300 ulp at
    // N = 384).  So j (2i + 1) is reduced mod 4G in integers and the cosine evaluated in long double, like twiddles(); each entry is
    // rounded to double once
    const long double half_pi_over_g = 3.141592653589793238462643383279502884L / (2.0L * G);
    for (int j = 0; j < N; ++j)
        for (int i = 0; i < G; ++i) {
            const long long r = (long long)j * (2 * i + 1) % (4LL * G);
            const long double c = cosl(half_pi_over_g * (long double)r), sg = (j & 1) ? -1.0L : 1.0L;
            Tf[(size_t)j * G + i] = (double)((2.0L / G) * c * (j == 0 ? 0.5L : 1.0L) * sg);
            Ti[(size_t)i * N + j] = (double)(sg * c);
        }
}
// (Ti Dz)^T (N x G): [j][z] = sum_m Ti[z][m] Dz[m][j], the non-zero terms added in the order of m
inline std::vector<double> ti_dz_transposed(const std::vector<double>& Ti, const std::vector<double>& Dz, int N, int G) {
    std::vector<double> t((size_t)N * G, 0.0);
    for (int j = 0; j < N; ++j) for (int m = 0; m < N; ++m) {
        const double d = Dz[(size_t)m * N + j];
        if (d != 0.0) for (int i = 0; i < G; ++i) t[(size_t)j * G + i] += Ti[(size_t)i * N + m] * d;
    }
    return t;
}
// keep the rows of u, v, rho and the last row of each derivative variable of S_n (6N x 3N): (3N + 3) x 3N (see pois_rank1_add)
inline void reduce_rows(const std::vector<cd>& s, int N, cd* dst) {
    const int n3 = 3 * N;
    std::copy(s.begin(), s.begin() + (size_t)n3 * n3, dst);
    for (int f = 0; f < 3; ++f) std::copy(&s[((size_t)(3 + f) * N + N - 1) * n3], &s[((size_t)(3 + f) * N + N - 1) * n3] + n3, dst + (size_t)(n3 + f) * n3);
}
// a reduced operator ((3N + 3) x 3N, rows and columns variable-major: the rows of u, v, rho and the three extra rows) -> mode-major
// ordering (index 3*mode + variable) of the square part, its HODLR factors (truncated at rel_tol * the largest entry), and the extra rows
// in the same column order
inline void hodlr_factor_reduced(const hodlr::Plan& plan, const cd* red, int N, double rel_tol, std::vector<cd>& perm, hodlr::Factors& f,
                                 std::vector<cd>& extras) {
    const int n3 = 3 * N;
    perm.resize((size_t)n3 * n3);
    extras.resize((size_t)3 * n3);
    double mx = 0.0;
    for (int v = 0; v < 3; ++v) for (int j = 0; j < N; ++j) {
        const cd* row = red + (size_t)(v * N + j) * n3;
        cd* prow = &perm[(size_t)(3 * j + v) * n3];
        for (int w = 0; w < 3; ++w) for (int i = 0; i < N; ++i) { prow[3 * i + w] = row[w * N + i]; mx = std::max(mx, std::abs(row[w * N + i])); }
    }
    for (int e = 0; e < 3; ++e) for (int w = 0; w < 3; ++w) for (int i = 0; i < N; ++i) extras[(size_t)e * n3 + 3 * i + w] = red[(size_t)(n3 + e) * n3 + w * N + i];
    hodlr::factor(plan, perm.data(), n3, rel_tol * mx, f);
}

}  // namespace tau
}  // namespace smo
