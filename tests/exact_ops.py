"""Two exact statements about the discrete KDyn scheme, as plain NumPy (shared by test_kdyn_exact_cpu.py, which pins them on the oracle, and
test_kdyn_exact_gpu.py, which demands them of the kernels).  Neither needs the oracle.

A.  For fixed B0, B_n is a polynomial of degree n in U, so along U + t d the cost J(t) — Final or Integrated — is a polynomial of degree 2n,
    and the central stencil on t = +-1 .. +-n with the weights exact through that degree returns J'(0) EXACTLY:
        <g, d> = sum_j w_j (J(+j d) - J(-j d))
    for the Discrete adjoint and every d that is solenoidal, mean-free and band-limited to |k_i| <= kmax (the adjoint projects, and the k = 0
    mode carries the constraint's sign flip).  In B0 the cost is quadratic: n = 1.  A plane wave a cos(k.x + phi), a perp k, is such a
    direction and reads ONE Fourier coefficient of the gradient: a needle in spectral space.

B.  With a uniform flow U = c no mode talks to another: N^ = i [c (k.B^) - B^ (k.c)] and
        B^_{n+1}(k) = P_k(beta B^_n + N^) / alpha - k (k.B^_n) / k^2,      B^_{n+1}(0) = -B^_n(0),      alpha, beta = 1/dt +- k^2 / 2Rm
    (oracle/kdyn.py cnab_update), for ANY B0 — non-solenoidal and non-zero-mean parts included.  uniform_flow_steps evaluates it in
    np.longdouble.

Vectors are the flat [3][G][G][G] ones of the callbacks, z fastest; <x, y> is Inner_Prod_3, the sum over components of the grid mean.
"""
from fractions import Fraction

import numpy as np


def stencil_weights(n):
    """w_1 .. w_n with sum_j w_j j^(2i+1) = delta_i0 / 2 for i = 0 .. n-1: sum_j w_j (p(j) - p(-j)) = p'(0) for every polynomial p of degree
    <= 2n.  Solved in rational arithmetic (w_j = (-1)^(j+1) n!^2 / (j (n-j)! (n+j)!)), returned as floats."""
    n = int(n)
    A = [[Fraction(j) ** (2 * i + 1) for j in range(1, n + 1)] + [Fraction(1 if i == 0 else 0, 2)] for i in range(n)]
    for col in range(n):                                   # Gauss-Jordan on exact fractions
        piv = next(r for r in range(col, n) if A[r][col] != 0)
        A[col], A[piv] = A[piv], A[col]
        A[col] = [v / A[col][col] for v in A[col]]
        for r in range(n):
            if r != col and A[r][col] != 0:
                A[r] = [v - A[r][col] * p for v, p in zip(A[r], A[col])]
    return [float(A[r][n]) for r in range(n)]


def stencil_derivative(w, Jp, Jm):
    """sum_j w_j (J(+j) - J(-j)); Jp[j-1] = J(+j d), Jm[j-1] = J(-j d)."""
    return sum(wj * (p - m) for wj, p, m in zip(w, Jp, Jm))


def stencil_scale(w, Jp, Jm):
    """sum_j |w_j| (|J(+j)| + |J(-j)|): what a relative error of the J carries into the stencil."""
    return sum(abs(wj) * (abs(p) + abs(m)) for wj, p, m in zip(w, Jp, Jm))


def inner(x, y, G):
    """Inner_Prod_3 on the host."""
    return float(np.dot(np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)) / float(G) ** 3)


JTOL, GTOL = 1e-12, 1e-11                 # test_symmetry_gpu.py: "same arithmetic, other summation order" on J (relative) and on a gradient (rel)
RTOL = 1e-6                               # test_kdyn_gpu.py: the norm tolerance of the oracle comparisons
SHARE = 1e-8                              # the needle bound must stay below this share of |g| |d| (else it could not see a 1e-8 error)
ORACLE_UNIFORM_DEFECT = 1e-15             # statement B on the oracle (float64 through pocketfft), worst of Npts 8, 10, 16 over 9 steps: 9.6e-16
UNIFORM_FLOW = (0.7, -0.4, 0.25)          # the flow of the statement-B tests
UNIFORM_TOL = 32. * ORACLE_UNIFORM_DEFECT   # the device's per-element bound: 32 x for other butterfly orders and the fused products


def needle_defect(g, d, w, Jp, Jm, G):
    """(defect, bound, |g| |d|) of statement A for one direction: defect = |<g, d> - stencil|, bound = JTOL on every J the stencil reads plus
    GTOL on |g| |d| (the form of test_kdyn_cost_is_a_quadratic_form_in_B0).  G: the KDyn grid size (Inner_Prod_3), or the problem's own
    inner product as a callable (x, y) -> float (exact_grad_ops.py: SH23, Poiseuille)."""
    ip = G if callable(G) else (lambda x, y: inner(x, y, G))
    gd = np.sqrt(ip(g, g) * ip(d, d))
    defect = abs(ip(g, d) - stencil_derivative(w, Jp, Jm))
    return defect, JTOL * stencil_scale(w, Jp, Jm) + GTOL * gd, gd


def unit_needle(G, k, rs):
    """A plane wave of wavenumber k with a seeded amplitude perp k and a seeded phase, <d, d> = 1."""
    a = perp_amplitude(k, rs)
    return np.sqrt(2.) * plane_wave(G, k, a, rs.uniform(0., 2. * np.pi))


def plane_wave(G, k, a, phi=0.):
    """Component c is a[c] cos(k.x + phi) on the G^3 grid of the 2 pi box; flat [3][G][G][G].  Built from three complex 1-D tables (no host
    FFT; the table arguments are reduced modulo G in integers first)."""
    j = np.arange(G)
    ex, ey, ez = (np.exp(2j * np.pi * ((int(ki) * j) % G) / G) for ki in k)
    exy = (np.exp(1j * float(phi)) * ex)[:, None] * ey[None, :]
    w = exy.real[:, :, None] * ez.real[None, None, :]
    w -= exy.imag[:, :, None] * ez.imag[None, None, :]
    out = np.empty((3, G, G, G))
    for c in range(3):
        np.multiply(w, float(a[c]), out=out[c])
    return out.reshape(-1)


def perp_amplitude(k, rs):
    """A seeded unit vector a with a . k = 0."""
    k = np.asarray(k, dtype=float)
    while True:
        a = rs.standard_normal(3)
        a -= k * (a @ k) / (k @ k)
        if np.linalg.norm(a) > 0.1:
            a /= np.linalg.norm(a)
            return a - k * (a @ k) / (k @ k)               # (a second pass: a . k to rounding of the unit vector)


def needle_wavenumbers(kmax, seed=7):
    """Corners, edges and faces of the retained cube |k_i| <= kmax, two axis wavenumbers of length 1, one mixed and two seeded interior ones:
    never k = 0, every |k_i| <= kmax, negative ky and kz among them."""
    kmax = int(kmax)
    ks = [(kmax, kmax, kmax), (kmax, -kmax, kmax), (0, kmax, -kmax), (0, -kmax, 0), (kmax, 0, 0), (0, 0, 1), (1, 0, 0),
          (min(2, kmax), -1, kmax)]
    rs = np.random.RandomState(seed)
    lim = max(kmax - 1, 1)
    while len(ks) < 10:
        k = (int(rs.randint(0, lim + 1)), int(rs.randint(-lim, lim + 1)), int(rs.randint(-lim, lim + 1)))
        if k != (0, 0, 0) and k not in ks:
            ks.append(k)
    return ks


# the reduced lists of the sizes where every forward solve is a call of its own
def boundary_needles(kmax):
    return [(kmax, -kmax, kmax), (0, -kmax, 0)]


def few_needles(kmax):
    return boundary_needles(kmax) + [(0, 0, 1)]


def wavenumbers(Npts):
    """K (3, a, m, m) of the spectral snapshots: kx = 0 .. kmax, ky and kz = 0 .. kmax, -kmax .. -1."""
    kmax = (int(Npts) - 1) // 2
    kx = np.arange(kmax + 1, dtype=float)
    kc = np.concatenate([np.arange(0, kmax + 1), np.arange(-kmax, 0)]).astype(float)
    return np.stack(np.meshgrid(kx, kc, kc, indexing='ij'))


def mode_index(k, kmax):
    """Index of the wavenumber k (kx >= 0) in an (a, m, m) coefficient array."""
    m = 2 * kmax + 1
    return (int(k[0]), int(k[1]) % m, int(k[2]) % m)


def uniform_flow_steps(S0, K, c, Rm, dt, n):
    """Yield the snapshots 1 .. n that follow S0 (3, a, m, m) under the uniform flow c, mode by mode in np.longdouble (complex)."""
    L = np.longdouble
    K = np.asarray(K).astype(L)
    c = [L(v) for v in c]
    k2 = (K * K).sum(0)
    zero = (k2 == 0)
    k2s = np.where(zero, L(1), k2)
    half_D = k2 / (L(2) * L(Rm))
    alpha, beta = L(1) / L(dt) + half_D, L(1) / L(dt) - half_D
    kc = K[0] * c[0] + K[1] * c[1] + K[2] * c[2]
    B = np.asarray(S0).astype(np.clongdouble)
    for _ in range(int(n)):
        kB = (K * B).sum(0)
        r = beta * B + 1j * (np.stack([c[0] * kB, c[1] * kB, c[2] * kB]) - B * kc)
        B1 = (r - K * ((K * r).sum(0) / k2s)) / alpha - K * (kB / k2s)
        B1[:, zero] = -B[:, zero]
        B = B1
        yield B
