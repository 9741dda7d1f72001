"""The exact directional check of exact_ops.py (statement A) for the Discrete adjoints of SH23 and Poiseuille, as plain NumPy: shared by
test_gradients_exact_cpu.py, which pins it on the oracles and characterises where the reference's adjoints are NOT exact gradients, and
test_gradients_exact_gpu.py, which demands it of the kernels.  Nothing here needs the oracle.

Along X + t d the discrete cost is a polynomial in t, so the central stencil on t = +-1 .. +-m with the weights exact through degree 2m
(exact_ops.stencil_weights) returns J'(0) = <g, d> to rounding:

    SH23        u_n has degree 3^n in X, J = -dt sum_{n <= N} mean(u_n^2) degree 2 3^N:  m = 3^N, every N, every d (the forward solve
                truncates X to the Nc retained modes and the gradient has no content outside them, so a direction out of the band gives
                <g, d> = 0 and a stencil of 0);
    Poiseuille  one step is quadratic in the state, J (s = 0) degree 2 2^N:  m = 2^N.  TRUE FOR N = 1 ONLY and only for directions inside
                the de-aliased band kx < a, kz < Nz0: from the second step on the adjoint differentiates the stored u, w, rho where the
                forward products read the tau solve's own uz, wz, rz (the reference does the same), and J is blind to a direction out of
                the band while the gradient is not (test_gradients_exact_cpu.py measures both).

A direction is d = h |X| d_unit with <d_unit, d_unit> = 1 in the problem's own inner product, h = H = 0.1 unless a case says otherwise.
Needles are single coefficients: cos(2 pi k x / G + phi) on the SH23 grid, cos(2 pi kx i / Nx + phi) cos(kz arccos(-z_j)) in one velocity
component for Poiseuille.  The bound is exact_ops.needle_defect's: JTOL on every J the stencil reads plus GTOL on |g| |d|; it must stay below
SHARE = 1e-8 of |g| |d|.
"""
import numpy as np

from exact_ops import GTOL, JTOL, needle_defect, stencil_derivative, stencil_scale, stencil_weights

H = 0.1                                   # |d| / |X| of every direction
H_LADDER = (0.1, 0.3, 1.0)                # where a case cannot meet SHARE at H, the smallest of these that does
SH23_NORM2, POIS_NORM2 = 0.0725, 0.02     # <X, X> of the inputs (band_ops.NORM2)
SH23_BOX = (0., 12. * np.pi)
SH23_A = -0.3
POIS_LX = 4. * np.pi
# The mix-norm cost (s = 1) after one step does not depend on u (dx rho_0 = 0) and depends on w through rz_0 alone: the analytic derivative
# of the base profile in the forward solve, Dz rho_0 in the adjoint (the reference's choice).  On the oracle the w needles miss by 3e-4
# (24, 24), 2e-12 (30, 66), 1e-2 (18, 15), 8e-5 (42, 27) of |g| |d| at every step of the ladder, and |J| is so much larger than what varies
# that the bound is 1.6e-8 at h = 0.1, 5.4e-9 at 0.3, 1.6e-9 at 1.0.  No step qualifies (test_gradients_exact_cpu.py): no s = 1 device case.
POIS_MIXNORM_H = None
# SH23 Hessian identity: the smallest step of the ladder at which the restatement's bound is below SHARE (test_gradients_exact_cpu.py)
SH23_HESSIAN_H = 0.1


def degree_half_width(kind, n):
    """m: J along a line has degree 2 m after n steps."""
    return {"sh23": 3, "pois": 2}[kind] ** int(n)


# ---- inner products --------------------------------------------------------------------------------------------------------------------
def sh23_inner(x, y):
    """Inner_Prod of SH23: the grid mean."""
    return float(np.mean(np.asarray(x) * np.asarray(y)))


def pois_weights(Nx, Nz, Lx=POIS_LX):
    """weightMatrixDisc: first differences of the Gauss grid times Lx / Nx, (Nx, Nz)."""
    z = -np.cos(np.pi * (np.arange(Nz) + 0.5) / Nz)
    dz = np.empty(Nz)
    dz[0] = z[1] - z[0]
    dz[1:] = z[1:] - z[:-1]
    return np.tile(dz * (Lx / Nx), (Nx, 1))


def pois_inner_product(Nx, Nz, Lx=POIS_LX):
    """Inner_Prod_Discrete as a callable (x, y) -> (1/V) sum W (x_u y_u + x_w y_w), V = 2 Lx."""
    W2 = np.concatenate([pois_weights(Nx, Nz, Lx).ravel()] * 2) / (2. * Lx)

    def ip(x, y):
        return float(np.dot(np.asarray(x).reshape(-1) * W2, np.asarray(y).reshape(-1)))
    return ip


# ---- inputs and directions -------------------------------------------------------------------------------------------------------------
def white(size, seed, norm2, ip):
    """Seeded standard_normal scaled to <X, X> = norm2 (the draw of band_ops.white_input), read-only."""
    x = np.random.RandomState(seed).standard_normal(size)
    x *= np.sqrt(norm2 / ip(x, x))
    x.setflags(write=False)
    return x


def unit(d, ip):
    return d / np.sqrt(ip(d, d))


def scaled(d_unit, X, h, ip):
    """d = h |X| d_unit."""
    return (h * np.sqrt(ip(X, X))) * d_unit


def line_points(X, d, m):
    """X + d, X - d, X + 2 d, X - 2 d, .. X - m d: the 2 m points a stencil of half-width m reads."""
    return [X + s * j * d for j in range(1, m + 1) for s in (1., -1.)]


def line_defect(g, d, m, Js, ip):
    """needle_defect for the J of line_points, in that order."""
    return needle_defect(g, d, stencil_weights(m), Js[0::2], Js[1::2], ip)


def blind_defect(g, d, m, Js, ip):
    """A direction the cost cannot see: (|<g, d>|, |stencil|, bound, JTOL scale) — the first two must be <= the last two."""
    w = stencil_weights(m)
    _, bound, _ = needle_defect(g, d, w, Js[0::2], Js[1::2], ip)
    return abs(ip(g, d)), abs(stencil_derivative(w, Js[0::2], Js[1::2])), bound, JTOL * stencil_scale(w, Js[0::2], Js[1::2])


def sh23_wavenumbers(Npts, seed=7):
    """(in-band k, out-of-band k) on the 2 Npts grid: 0, 1, Nc // 2, Nc - 1 and two seeded interior ones; Nc + 2 and G / 2."""
    Nc, G = (Npts - 1) // 2 + 1, 2 * Npts
    ks = [0, 1, Nc // 2, Nc - 1]
    rs = np.random.RandomState(seed)
    while len(ks) < 6:
        k = int(rs.randint(2, Nc - 1))
        if k not in ks:
            ks.append(k)
    return ks, [Nc + 2, G // 2]


def sh23_directions(Npts, seed=7):
    """[(name, in_band, d_unit)]: the needles of sh23_wavenumbers with seeded phases and one white direction (the forward solve truncates
    it, the gradient is orthogonal to the rest: the identity holds for it as it stands)."""
    G = 2 * Npts
    inside, outside = sh23_wavenumbers(Npts, seed)
    rs = np.random.RandomState(seed + 1)
    j = np.arange(G)
    out = []
    for k in inside + outside:
        phi = rs.uniform(0.25, 1.25)                        # (away from the zeros of cos: k = 0 and k = G / 2 are cos(phi) times +-1)
        d = np.cos(2. * np.pi * ((k * j) % G) / G + phi)
        out.append(("k=%d" % k, k in inside, unit(d, sh23_inner)))
    out.append(("white", True, unit(rs.standard_normal(G), sh23_inner)))
    return out


def pois_band(Nx, Nz):
    """(a, Nz0): the de-aliased band is kx < a, kz < Nz0."""
    return (2 * Nx // 3) // 2, 2 * Nz // 3


def pois_wavenumbers(Nx, Nz, which="all", seed=7):
    """(in-band (kx, kz), out-of-band (kx, kz)): corners ("corners": only these), edge midpoints and two seeded interior points of
    [0, a-1] x [0, Nz0-1]; (a, 1) and (1, Nz0)."""
    a, Nz0 = pois_band(Nx, Nz)
    ks = [(0, 0), (a - 1, 0), (0, Nz0 - 1), (a - 1, Nz0 - 1)]
    if which == "all":
        ks += [(a // 2, 0), (a // 2, Nz0 - 1), (0, Nz0 // 2), (a - 1, Nz0 // 2)]
        rs = np.random.RandomState(seed)
        while len(ks) < 10:
            k = (int(rs.randint(1, a - 1)), int(rs.randint(1, Nz0 - 1)))
            if k not in ks:
                ks.append(k)
    return ks, [(a, 1), (1, Nz0)]


def pois_needle(Nx, Nz, comp, kx, kz, phi):
    """Component comp (0: u, 1: w) = cos(2 pi kx i / Nx + phi) cos(kz arccos(-z_j)), the other zero; flat [2][Nx][Nz]."""
    i, theta = np.arange(Nx), np.pi * (np.arange(Nz) + 0.5) / Nz            # arccos(-z_j) = pi (j + 1/2) / Nz on the ascending Gauss grid
    d = np.zeros((2, Nx, Nz))
    d[comp] = np.cos(2. * np.pi * ((kx * i) % Nx) / Nx + phi)[:, None] * np.cos(kz * theta)[None, :]
    return d.reshape(-1)


def pois_directions(Nx, Nz, comps="uw", which="all", seed=7):
    """[(name, in_band, d_unit)] for the components named."""
    ip = pois_inner_product(Nx, Nz)
    inside, outside = pois_wavenumbers(Nx, Nz, which, seed)
    rs = np.random.RandomState(seed + 1)
    out = []
    for c in comps:
        for kx, kz in inside + outside:
            d = pois_needle(Nx, Nz, "uw".index(c), kx, kz, rs.uniform(0.25, 1.25))
            out.append(("%s(%d,%d)" % (c, kx, kz), (kx, kz) in inside, unit(d, ip)))
    return out


def pois_band_project(v, Nx, Nz, comps="uw"):
    """Both components of a flat vector cut to the de-aliased band (x: real FFT; z: the Chebyshev series on the Gauss grid, as matrices);
    a component not named in comps is set to zero."""
    a, Nz0 = pois_band(Nx, Nz)
    theta = np.pi * (np.arange(Nz) + 0.5) / Nz
    C = np.cos(np.arange(Nz0)[:, None] * theta[None, :])                   # (Nz0, Nz): T_k at the grid, up to the sign (-1)^k
    scale = np.where(np.arange(Nz0) == 0, 1., 2.) / Nz
    Pz = C.T @ (scale[:, None] * C)                                        # (Nz, Nz), symmetric
    f = np.asarray(v, dtype=float).reshape(2, Nx, Nz)
    F = np.fft.rfft(f, axis=1)
    F[:, a:] = 0.
    out = np.fft.irfft(F, n=Nx, axis=1) @ Pz
    for c in "uw":
        if c not in comps:
            out["uw".index(c)] = 0.
    return out.reshape(-1)


# ---- the Hessian identity of SH23 --------------------------------------------------------------------------------------------------------
def hessian_line_defect(W, HV, gp, gm, m, ip):
    """Along X + t V the SH23 Discrete gradient is a polynomial of degree 2 3^n - 1 <= 2 m, so
        <W, H V> = sum_j w_j (<g(X + j V), W> - <g(X - j V), W>)
    exactly.  gp[j-1] = g(X + j V), gm[j-1] = g(X - j V).  Returns (defect, bound, |HV| |W|), bound = GTOL on every gradient the stencil
    reads (times |W|) plus GTOL on |HV| |W|."""
    w = stencil_weights(m)
    nW, nH = np.sqrt(ip(W, W)), np.sqrt(ip(HV, HV))
    est = stencil_derivative(w, [ip(p, W) for p in gp], [ip(q, W) for q in gm])
    size = stencil_scale(w, [np.sqrt(ip(p, p)) for p in gp], [np.sqrt(ip(q, q)) for q in gm])
    return abs(ip(W, HV) - est), GTOL * size * nW + GTOL * nH * nW, nH * nW
