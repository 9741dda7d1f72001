"""The Chebyshev transforms of SHB23 and of Poiseuille Discrete as closed-form matrices in np.longdouble, the inputs that pick out single
columns of them, and a defect measured in units of the rounding of the map itself (shared by test_transforms_exact_cpu.py, which shows on
the oracle alone that these matrices are the reference's maps and where the tolerances come from, and test_transforms_exact_gpu.py, which
holds the kernels to them).

Every other check of these maps feeds one random vector and judges one norm over the whole result (rel < 1e-13 / 1e-12): a single matrix
entry off by 1e-11 of its column passes.  Here every map is a matrix M known in closed form, and

    defect(got, M, x) = max_i |got_i - (M x)_i| / (u max_i (|M| |x|)_i),        u = 2^-52

so for a needle x = e_j the result is column j of the map, judged entry by entry against the largest entry of that column.

SHB23, N grid points, theta_i = pi (i + 1/2) / N:
    transform               F[k, i]  = eps_k (-1)^k cos(k theta_i) / N        (eps_0 = 1, eps_k = 2)
    transformInverse        Bi[i, k] = (-1)^k cos(k theta_i)
    transformAdjoint        F^T                 transformInverseAdjoint     Bi^T
Poiseuille Discrete, Nx x Nz, a = Nx / 2 carried wavenumbers, E[n, x] = exp(-2 pi i ((n x) mod Nx) / Nx), w_0 = 1, w_n = 2:
    transform               E g F^T / Nx                       transformInverseAdjoint     E g Bi
    transformInverse        Re(E^H diag(w) (c Bi^T))           transformAdjoint            Re(E^H diag(w) (c F)) / Nx
(coefficient inputs have a real row n = 0).  Every cosine is taken of an argument reduced in integers first (k (2i + 1) mod 4N, n x mod Nx),
pi = 4 arctan(1) in longdouble.

Imports numpy only (and the pure-Python any_plan of test_any_fft_model.py).
"""
import functools

import numpy as np

from test_any_fft_model import any_plan

LD = np.longdouble
U = 2.0 ** -52
PI = 4 * np.arctan(LD(1))
SEED = 42
MAPS = ("transform", "transformInverse", "transformAdjoint", "transformInverseAdjoint")

# ---- tolerances (ulp, in the sense of defect()) -------------------------------------------------------------------------------------------
# 8 x the oracle's worst defect over the tables below, rounded up (test_transforms_exact_cpu.py asserts oracle <= TOL_ULP / 8).  The
# device computes the same maps by other algorithms (Stockham stages with direct sums of up to 1021 terms, Makhoul twiddles, MFMA sums over
# up to 198 terms) whose rounding constants differ from pocketfft's by a small factor; every defect these tests exist for (a wrong twiddle
# index, a sign, a dropped or misplaced element, a tile edge) is at least 1e-3 of a column maximum: above 1e12 ulp.
# Measured on the oracle (scipy's pocketfft, NumPy's FFT):
#     SHB23      needle  7.94 (N = 998, transformAdjoint, column 499; 6.20 at 1021, 5.96 at 257)    dense  1.53 (N = 13, transform, alternating)
#     Poiseuille needle  4.10 (24 x 24, transformAdjoint, n = 1, k = 23)                            dense  1.78 (66 x 63, transformAdjoint, alternating)
TOL_ULP = {("shb23", "needle"): 64, ("shb23", "dense"): 13, ("pois", "needle"): 33, ("pois", "dense"): 15}


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------
SHB_INSTANTIATED = [64, 96, 128, 192, 256, 384, 512, 768, 1024]          # dct2 / dct3 of csrc/shb23.hip at half these lengths
SHB_RUNTIME = [49, 77, 121, 125, 143, 169, 243, 250, 257, 289, 343, 509, 961, 998, 1000, 1015, 1021, 1022, 1023]
SHB_LENGTHS = sorted(set(range(4, 49)) | set(SHB_INSTANTIATED) | set(SHB_RUNTIME))
SHB_ANY_FORCED = [64, 768, 1024]                                         # instantiated lengths sent through any_plan (SMO_SHB_ANY=1)
SHB_ALL_NEEDLES_UP_TO = 64

POIS_XFFT = [24, 30, 36, 48, 60, 96, 192, 384, 768]                      # Nx with an x-FFT instantiation (csrc/pois.hip)
POIS_TILE = 32                                                           # pois_gemm: 32 x 32 tiles, 32-deep K slices
POIS_SHAPES = [(12, 12), (18, 15), (24, 24), (30, 33), (42, 27), (66, 63), (96, 66), (102, 99), (198, 129)]
POIS_ALL_NEEDLES_UP_TO = 18 * 15


def shb_uses_any_plan(N):
    return N % 2 == 1 or N not in SHB_INSTANTIATED


def shb_needles(N):
    if N <= SHB_ALL_NEEDLES_UP_TO:
        return list(range(N))
    fixed = {0, 1, 2, 3, N // 2 - 1, N // 2, N // 2 + 1, N - 3, N - 2, N - 1}
    return sorted(fixed | set(np.random.RandomState(N).choice(N, 6, replace=False).tolist()))


def _marks(n, with_last_but_one):
    m = {0, 1, n // 2, n - 1} | {i for i in (31, 32, 33) if i < n}
    return sorted(m | {n - 2} if with_last_but_one else m)


def pois_needles(Nx, Nz, coefficient):
    """[(row, column)]: grid positions (x, z), or coefficient positions (n, k) with n < Nx / 2."""
    rows = Nx // 2 if coefficient else Nx
    if Nx * Nz <= POIS_ALL_NEEDLES_UP_TO:
        return [(r, c) for r in range(rows) for c in range(Nz)]
    return [(r, c) for r in _marks(rows, False) for c in _marks(Nz, True)]


def pois_gemm_dims(Nx, Nz):
    """(M, N, K) of the products a standalone transform runs: x then z to coefficients, z then x to the grid."""
    m = 2 * (Nx // 2)
    return [(m, Nz, Nx), (m, Nz, Nz), (Nx, Nz, m)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _frozen(x):
    x.setflags(write=False)
    return x


def shb_dense_inputs(N):
    """[(label, x)]: seeded white noise, the constant 1, the alternating +-1."""
    return [("white", _frozen(np.random.RandomState(SEED).standard_normal(N))), ("ones", _frozen(np.ones(N))),
            ("alternating", _frozen((-1.) ** np.arange(N)))]


def pois_dense_inputs(Nx, Nz, coefficient):
    """Grid arrays (Nx, Nz), or complex coefficient arrays (Nx / 2, Nz) with a real row n = 0 (both parts of the other rows carry the pattern)."""
    rs = np.random.RandomState(SEED)
    if not coefficient:
        alt = (-1.) ** (np.arange(Nx)[:, None] + np.arange(Nz)[None, :])
        return [("white", _frozen(rs.standard_normal((Nx, Nz)))), ("ones", _frozen(np.ones((Nx, Nz)))), ("alternating", _frozen(alt))]
    a = Nx // 2
    out = []
    for label, c in (("white", rs.standard_normal((a, Nz)) + 1j * rs.standard_normal((a, Nz))), ("ones", np.full((a, Nz), 1. + 1.j)),
                     ("alternating", (1. + 1.j) * (-1.) ** (np.arange(a)[:, None] + np.arange(Nz)[None, :]))):
        c[0] = c[0].real
        out.append((label, _frozen(c)))
    return out


def hermitian_full(Nx, c):
    """(a, Nz) coefficients of the wavenumbers 0..a-1 -> the oracle's full spectrum (0..kmax, -kmax..-1) of a real field."""
    a = Nx // 2
    assert Nx % 2 == 0 and c.shape[0] == a
    full = np.concatenate([c, np.conj(c[:0:-1])])
    full[0] = full[0].real
    return full


# ---- matrices -------------------------------------------------------------------------------------------------------------------------------
def _cheb_cos(N):
    """C[k, i] = cos(k theta_i)."""
    k, i = np.arange(N, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]
    return np.cos(PI * ((k * (2 * i + 1)) % (4 * N)).astype(LD) / (2 * N))


@functools.lru_cache(maxsize=2)
def shb_matrices(N):
    """(F, Bi, F^T, Bi^T) in the order of MAPS, longdouble."""
    k = np.arange(N)[:, None]
    sc = np.where(k % 2 == 1, -1, 1).astype(LD) * _cheb_cos(N)
    F = np.where(k == 0, 1, 2).astype(LD) * sc / N
    Bi = np.ascontiguousarray(sc.T)
    return F, Bi, F.T, Bi.T


@functools.lru_cache(maxsize=2)
def pois_factors(Nx, Nz):
    """(Er, Ei, w, Z): E = Er + i Ei (a, Nx); Z[which] the z factor applied from the right: F^T / Nx (z, k), Bi^T (k, z), F / Nx (k, z), Bi (z, k)."""
    a = Nx // 2
    n, x = np.arange(a, dtype=np.int64)[:, None], np.arange(Nx, dtype=np.int64)[None, :]
    ph = 2 * PI * ((n * x) % Nx).astype(LD) / Nx
    F, Bi, _, _ = shb_matrices(Nz)
    w = np.where(np.arange(a) == 0, 1, 2).astype(LD)[:, None]
    return np.cos(ph), -np.sin(ph), w, (F.T / Nx, Bi.T, F / Nx, Bi)


# ---- defects --------------------------------------------------------------------------------------------------------------------------------
def defect(got, M, x):
    """max_i |got_i - (M x)_i| / (u max_i (|M| |x|)_i)."""
    x = np.asarray(x, dtype=LD)
    return float(np.abs(np.asarray(got, dtype=LD) - M @ x).max() / (U * (np.abs(M) @ np.abs(x)).max()))


def needle_defect(got, M, j):
    """defect(got, M, e_j): against column j, in units of its largest entry."""
    col = M[:, j]
    return float(np.abs(np.asarray(got, dtype=LD) - col).max() / (U * np.abs(col).max()))


def _parts(z):
    z = np.asarray(z)
    return z.real.astype(LD), z.imag.astype(LD)


def pois_expected(Nx, Nz, which, x):
    """(real part, imaginary part or None, abs-sum |M| |x|) of map `which` applied to a dense input, from the separable factors."""
    Er, Ei, w, Zs = pois_factors(Nx, Nz)
    Z = Zs[which]
    if which in (0, 3):
        g = np.asarray(x, dtype=LD)
        t = g @ Z
        return Er @ t, Ei @ t, (np.abs(g) @ np.abs(Z)).sum(axis=0)           # |E| = 1: the same abs-sum for every n, one per k
    cr, ci = _parts(x)
    ref = Er.T @ (w * (cr @ Z)) + Ei.T @ (w * (ci @ Z))
    return ref, None, np.abs(Er).T @ (w * (np.abs(cr) @ np.abs(Z))) + np.abs(Ei).T @ (w * (np.abs(ci) @ np.abs(Z)))


def pois_needle_expected(Nx, Nz, which, r, c, imaginary=False):
    """The same for a needle: a 1 at grid position (r, c), or a 1 (imaginary: an i) at coefficient position (r, c); rank one."""
    Er, Ei, w, Zs = pois_factors(Nx, Nz)
    Z = Zs[which]
    if which in (0, 3):
        return Er[:, r, None] * Z[c, None, :], Ei[:, r, None] * Z[c, None, :], np.abs(Z[c]).max()
    ref = w[r, 0] * (Ei if imaginary else Er)[r, :, None] * Z[c, None, :]
    return ref, None, np.abs(ref).max()


def _pois_defect(got, re, im, scale):
    gr, gi = _parts(got)
    err = np.abs(gr - re) if im is None else np.hypot(gr - re, gi - im)
    assert im is not None or not np.any(gi)
    return float(err.max() / (U * np.max(scale)))


# ---- a whole length / shape: the worst defect per input kind ------------------------------------------------------------------------------
class Worst(dict):
    """{kind: (defect, where)}"""
    def see(self, kind, d, where):
        if not d <= self.get(kind, (-1.,))[0]:                      # (a NaN takes the place, too)
            self[kind] = (d, where)


def shb_worst(N, fns):
    """fns: the four maps in the order of MAPS, each vector -> vector.  {"needle": (worst defect, (map, column)), "dense": (.., (map, label))}."""
    worst = Worst()
    for name, M, f in zip(MAPS, shb_matrices(N), fns):
        for j in shb_needles(N):
            e = np.zeros(N)
            e[j] = 1.
            worst.see("needle", needle_defect(f(e), M, j), (name, j))
        for label, x in shb_dense_inputs(N):
            worst.see("dense", defect(f(x), M, x), (name, label))
    return worst


@functools.lru_cache(maxsize=2)
def _pois_dense_refs(Nx, Nz):
    return [[(label, x) + pois_expected(Nx, Nz, which, x) for label, x in pois_dense_inputs(Nx, Nz, which in (1, 2))] for which in range(4)]


def pois_worst(Nx, Nz, fns):
    """fns in the order of MAPS: transform and transformInverseAdjoint (Nx, Nz) real -> (Nx / 2, Nz) complex, the other two back."""
    worst = Worst()
    a = Nx // 2
    dense = _pois_dense_refs(Nx, Nz)
    for which, (name, f) in enumerate(zip(MAPS, fns)):
        coefficient = which in (1, 2)
        for r, c in pois_needles(Nx, Nz, coefficient):
            for imaginary in ((False, True) if coefficient and r > 0 else (False,)):
                e = np.zeros((a, Nz), dtype=complex) if coefficient else np.zeros((Nx, Nz))
                e[r, c] = 1j if imaginary else 1.
                worst.see("needle", _pois_defect(f(e), *pois_needle_expected(Nx, Nz, which, r, c, imaginary)), (name, r, c, "i" if imaginary else "1"))
        for label, x, re, im, scale in dense[which]:
            worst.see("dense", _pois_defect(f(x), re, im, scale), (name, label))
    return worst


# ---- the oracle's maps in the calling convention of the device's ------------------------------------------------------------------------------
def oracle_shb_fns():
    from oracle import shb23 as osh
    return [osh.transform, osh.transformInverse, osh.transformAdjoint, osh.transformInverseAdjoint]


def oracle_pois_fns(Nx, Nz):
    from oracle.poiseuille import PoiseuilleOracle
    o = PoiseuilleOracle(Nx, Nz)
    a = Nx // 2
    assert o.ax == a

    def real_field(v):
        assert np.abs(v.imag).max() <= 1e-12 * max(np.abs(v.real).max(), 1e-300)
        return v.real
    return [lambda g: o.transform(g)[:a], lambda c: real_field(o.transformInverse(hermitian_full(Nx, c))),
            lambda c: real_field(o.transformAdjoint(hermitian_full(Nx, c))), lambda g: o.transformInverseAdjoint(g)[:a]]
