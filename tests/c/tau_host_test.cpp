// CPU test of spheremanopt_amd/csrc/tau_host.hpp: the Chebyshev-tau operators of SHB23 and Poiseuille, without a GPU.
//   tau_host_test exact                      the suite's cases of the four checks below; prints one line per check, exits non-zero on a failure
//   tau_host_test lu Nz [Nz ...]             check 1 for the Poiseuille systems at other sizes (by hand: the workload's Nz = 192, 384 take minutes)
//   tau_host_test dump shb N FILE            S (N x N doubles, row-major) as raw bytes
//   tau_host_test dump solve Nz n adj FILE   S_n (6Nz x 3Nz complex) of the forward (adj = 0) or the adjoint (adj = 1) IVP
//   tau_host_test dump mixnorm Nz n FILE     S^MN_n (2Nz x Nz complex)
// Checks:  1. lu_solve (pivots and eliminates inside a window, updates inside a per-row column bound) == a plain partial-pivot LU that
//             searches every row and updates every column, byte for byte, on one assembled system;
//          2. Pre * D == PD entry by entry (every term is a small integer or a half);
//          3. max |Tf Ti - I| <= 4 N eps;
//          4. every entry of Tf (N x G) and Ti (G x N) within 1 ulp (of 2 / G and of 1) of cos(pi j (2i + 1) / (2G)) in long double, the
//             argument folded into the first octant in integers (so neither side of the comparison sees an argument above pi / 4).
// Parameters are the oracle's defaults: Re = Pe = 500, Ri = 0.05, a0 = 1 / dt = 200, k = n / 2 (Lx = 4 pi); SHB23: dt = 1e-2, a = -0.1 on (-20, 20).
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "hodlr.hpp"
#include "tau_host.hpp"

using namespace smo::tau;

constexpr double RE = 500.0, PE = 500.0, RI = 0.05, A0 = 200.0;
constexpr double SHB_DT = 1e-2, SHB_A = -0.1, SHB_Z0 = -20.0, SHB_Z1 = 20.0;

// plain LU with partial pivoting: every row at or below k is a pivot candidate (lowest index first, replaced only by a strictly larger
// modulus, as in lu_solve), every row below k with a non-zero multiplier is eliminated over ALL columns, and the back substitution runs
// over all columns (skipping exact zeros changes no bit: x - 0 * y == x)
template <class T> static int plain_lu(int n, std::vector<T>& A, int m, std::vector<T>& B) {
    auto at = [&](int r, int c) -> T& { return A[(size_t)r * n + c]; };
    for (int k = 0; k < n; ++k) {
        int p = -1; double best = 0.0;
        for (int r = k; r < n; ++r) { const double v = std::abs(at(r, k)); if (v > best) { best = v; p = r; } }
        if (p < 0) return k;
        if (p != k) {
            for (int c = 0; c < n; ++c) std::swap(at(k, c), at(p, c));
            for (int j = 0; j < m; ++j) std::swap(B[(size_t)k * m + j], B[(size_t)p * m + j]);
        }
        const T piv = at(k, k);
        for (int r = k + 1; r < n; ++r) {
            const T f = at(r, k);
            if (f == T(0)) continue;
            const T l = f / piv;
            at(r, k) = 0;
            for (int c = k + 1; c < n; ++c) at(r, c) -= l * at(k, c);
            for (int j = 0; j < m; ++j) B[(size_t)r * m + j] -= l * B[(size_t)k * m + j];
        }
    }
    for (int k = n - 1; k >= 0; --k) {
        for (int c = k + 1; c < n; ++c) {
            const T u = at(k, c);
            if (u == T(0)) continue;
            for (int j = 0; j < m; ++j) B[(size_t)k * m + j] -= u * B[(size_t)c * m + j];
        }
        const T inv = 1.0 / at(k, k);
        for (int j = 0; j < m; ++j) B[(size_t)k * m + j] *= inv;
    }
    return -1;
}

// one assembled system, two solvers: true when both succeed and the solutions are equal byte for byte
template <class T> static bool same_solution(const char* what, int p0, int p1, int p2, int n, int nb, int win, const std::vector<T>& A, int m, const std::vector<T>& B) {
    std::vector<T> A1 = A, B1 = B, A2 = A, B2 = B;
    const int c1 = lu_solve(n, nb, win, A1, m, B1), c2 = plain_lu(n, A2, m, B2);
    const bool ok = c1 < 0 && c2 < 0 && std::memcmp(B1.data(), B2.data(), B1.size() * sizeof(T)) == 0;
    if (!ok) {
        size_t bad = 0; double worst = 0.0;
        for (size_t i = 0; i < B1.size(); ++i) if (std::memcmp(&B1[i], &B2[i], sizeof(T)) != 0) { ++bad; worst = std::max(worst, (double)std::abs(B1[i] - B2[i])); }
        std::printf("FAIL lu %s %d %d %d: singular columns %d / %d, %zu of %zu entries differ, largest difference %.3e\n", what, p0, p1, p2, c1, c2, bad,
                    B1.size(), worst);
    }
    return ok;
}

static int check_lu_pois(const std::vector<int>& sizes) {
    int fails = 0, cases = 0;
    std::vector<cd> A, B;
    for (int N : sizes) {
        const Cheb ch(N);
        for (int n : {0, 1, 3})
            for (int adj = 0; adj < 2; ++adj) {
                assemble_solve_system(ch, n, 0.5 * n, A0, RE, PE, RI, adj != 0, A, B);
                fails += !same_solution("solve (Nz, n, adjoint)", N, n, adj, solve_unknowns(N, n), 7 * (N - 1), SOLVE_WIN, A, 3 * N, B); ++cases;
            }
        for (int n : {0, 2}) {
            assemble_mixnorm_system(ch, n, 0.5 * n, A, B);
            fails += !same_solution("mixnorm (Nz, n, -)", N, n, 0, mixnorm_unknowns(N, n), 2 * (N - 1), MIXNORM_WIN, A, N, B); ++cases;
        }
    }
    std::printf("%s lu poiseuille: %d cases, %d differ\n", fails ? "FAIL" : "ok", cases, fails);
    return fails;
}
static int check_lu_shb() {
    int fails = 0, cases = 0;
    std::vector<double> A, B;
    for (int N : {4, 8, 33, 64, 200}) {
        shb_assemble(N, SHB_DT, SHB_A, SHB_Z0, SHB_Z1, A, B);
        fails += !same_solution("shb (N, -, -)", N, 0, 0, 4 * N, 4 * N, 4 * N, A, N, B); ++cases;
    }
    std::printf("%s lu shb23: %d cases, %d differ\n", fails ? "FAIL" : "ok", cases, fails);
    return fails;
}
static int check_pre_d() {
    int fails = 0;
    for (int N : {12, 33, 96, 384}) {
        const Cheb ch(N);
        size_t bad = 0;
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) {
                double s = 0.0;
                for (int m = 0; m < N; ++m) s += ch.Pre[(size_t)i * N + m] * ch.D[(size_t)m * N + j];
                if (s != ch.PD[(size_t)i * N + j]) ++bad;
            }
        if (bad) { std::printf("FAIL Pre * D != PD at N = %d: %zu entries\n", N, bad); ++fails; }
    }
    std::printf("%s Pre * D == PD\n", fails ? "FAIL" : "ok");
    return fails;
}
static int check_pair() {
    int fails = 0;
    double worst = 0.0;                                        // in units of N eps
    for (int N : {12, 33, 96, 192, 384}) {
        std::vector<double> Tf, Ti, z;
        cheb_pair(N, N, Tf, Ti, z);
        double mx = 0.0;
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j) {
                double s = 0.0;
                for (int g = 0; g < N; ++g) s += Tf[(size_t)i * N + g] * Ti[(size_t)g * N + j];
                mx = std::max(mx, std::abs(s - (i == j ? 1.0 : 0.0)));
            }
        worst = std::max(worst, mx / (N * DBL_EPSILON));
        if (!(mx <= 4.0 * N * DBL_EPSILON)) { std::printf("FAIL max|Tf Ti - I| = %.3e = %.2f N eps at N = %d\n", mx, mx / (N * DBL_EPSILON), N); ++fails; }
    }
    std::printf("%s max|Tf Ti - I| <= 4 N eps (largest %.2f N eps)\n", fails ? "FAIL" : "ok", worst);
    return fails;
}
// cos(pi r / (2G)) for an integer r: r mod 4G, folded by the symmetries of the cosine to an angle in [0, pi / 4]
static long double folded_cos(long long r, int G) {
    const long double q = 3.141592653589793238462643383279502884L / (2.0L * G);
    r %= 4LL * G;
    if (r > 2LL * G) r = 4LL * G - r;                          // cos(2 pi - t) = cos t
    long double sg = 1.0L;
    if (r > G) { r = 2LL * G - r; sg = -1.0L; }                // cos(pi - t) = -cos t
    return sg * (2 * r > G ? sinl(q * (long double)(G - r)) : cosl(q * (long double)r));      // cos t = sin(pi / 2 - t)
}
static int check_entries() {
    int fails = 0;
    double worst_f = 0.0, worst_i = 0.0;                       // in ulp of 2 / G and of 1
    const int sizes[][2] = {{12, 12}, {33, 33}, {96, 96}, {99, 99}, {192, 192}, {384, 384}, {12, 18}, {96, 144}, {384, 576}};      // G = N, and 3N / 2
    for (const auto& ng : sizes) {
        const int N = ng[0], G = ng[1];
        std::vector<double> Tf, Ti, z;
        cheb_pair(N, G, Tf, Ti, z);
        const double ulp_f = std::nextafter(2.0 / G, 1.0) - 2.0 / G;
        double mf = 0.0, mi = 0.0;
        for (int j = 0; j < N; ++j)
            for (int i = 0; i < G; ++i) {
                const long double c = ((j & 1) ? -1.0L : 1.0L) * folded_cos((long long)j * (2 * i + 1), G);
                mf = std::max(mf, (double)fabsl((long double)Tf[(size_t)j * G + i] - (2.0L / G) * (j == 0 ? 0.5L : 1.0L) * c) / ulp_f);
                mi = std::max(mi, (double)fabsl((long double)Ti[(size_t)i * N + j] - c) / DBL_EPSILON);
            }
        worst_f = std::max(worst_f, mf); worst_i = std::max(worst_i, mi);
        if (!(mf <= 1.0 && mi <= 1.0)) { std::printf("FAIL entries at N = %d, G = %d: Tf off by %.1f ulp of 2 / G, Ti by %.1f ulp of 1\n", N, G, mf, mi); ++fails; }
    }
    std::printf("%s entries of Tf, Ti within 1 ulp of the closed form (largest %.2f ulp of 2 / G, %.2f ulp of 1)\n", fails ? "FAIL" : "ok", worst_f, worst_i);
    return fails;
}

template <class T> static int write_file(const char* path, const std::vector<T>& v) {
    std::FILE* f = std::fopen(path, "wb");
    if (!f) { std::perror(path); return 1; }
    const size_t n = std::fwrite(v.data(), sizeof(T), v.size(), f);
    return (std::fclose(f) == 0 && n == v.size()) ? 0 : 1;
}
static int dump(int argc, char** argv) {
    const std::string kind = argc > 2 ? argv[2] : "";
    if (kind == "shb" && argc == 5) {
        std::vector<double> S;
        if (shb_tau_operator(atoi(argv[3]), SHB_DT, SHB_A, SHB_Z0, SHB_Z1, S) >= 0) return 1;
        return write_file(argv[4], S);
    }
    if (kind == "solve" && argc == 7) {
        const int n = atoi(argv[4]);
        std::vector<cd> S;
        if (build_solve_map(Cheb(atoi(argv[3])), n, 0.5 * n, A0, RE, PE, RI, S, atoi(argv[5]) != 0) >= 0) return 1;
        return write_file(argv[6], S);
    }
    if (kind == "mixnorm" && argc == 6) {
        const int n = atoi(argv[4]);
        std::vector<cd> S;
        if (build_mixnorm_map(Cheb(atoi(argv[3])), n, 0.5 * n, S) >= 0) return 1;
        return write_file(argv[5], S);
    }
    std::fprintf(stderr, "usage: tau_host_test dump shb N FILE | dump solve Nz n adj FILE | dump mixnorm Nz n FILE\n");
    return 2;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "exact") return (check_lu_pois({12, 15, 24, 33, 48, 96}) + check_lu_shb() + check_pre_d() + check_pair() + check_entries()) ? 1 : 0;
    if (mode == "lu" && argc > 2) {
        std::vector<int> sizes;
        for (int i = 2; i < argc; ++i) sizes.push_back(atoi(argv[i]));
        return check_lu_pois(sizes) ? 1 : 0;
    }
    if (mode == "dump") return dump(argc, argv);
    std::fprintf(stderr, "usage: tau_host_test exact | lu Nz ... | dump ...\n");
    return 2;
}
