"""The reductions that feed the optimiser (kd_dot, kd_energy, sh23_inner_kernel, shb_inner_kernel, pois_dot) and the element-wise
vec_axpby, on data for which ANY correct summation order gives the same floating-point answer: small integers (every partial sum is an
integer below 2^53), single non-zero entries ("needles": one element counted twice, or not at all, changes the result by a whole
term), and spectra with power-of-two amplitudes.  Vector lengths run past one pass of every grid-stride loop.  The oracle checks of the
same kernels hold to 1e-6; one element of 21 million dropped is 5e-8.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import test_devvec_gpu as devvec_tests
from spheremanopt_amd import _capi, kdyn, poiseuille as pz, sh23, shb23
from spheremanopt_amd.devvec import DeviceVector

pytestmark = pytest.mark.gpu


def _ulps(a, b):
    return abs(a - b) / np.spacing(abs(b))


def _integers(rs, n):
    return rs.randint(-8, 9, n).astype(np.float64)


def _int_dot(x, y):
    return int(np.dot(x.astype(np.int64), y.astype(np.int64)))


# ---- KDyn Inner_Prod_3 (kd_dot: 1024 workgroups of 256 lanes, one pair of elements per lane and pass) -----------------------------------
_KD_PASS = 2 * 1024 * 256            # elements of one grid-stride pass


def _kd_needles(n):
    idx = [0, n - 2, n - 1]
    for k in (1, 2):
        idx += [i for i in (_KD_PASS * k - 1, _KD_PASS * k, _KD_PASS * k + 1) if i < n]
    return idx


# G = 9, 33: n = 3 G^3 is odd (a tail element; members 1 and 2 of a batch are only 8-byte aligned); G = 66, 96: more than one pass
@pytest.mark.parametrize("N", [6, 22, 16, 44, 64])
@pytest.mark.parametrize("batch", [1, 3])
def test_kdyn_inner_product_is_exact_on_integers(N, batch):
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(1., 1e-3, 1, "Final", batch=batch)
    n, G3 = ctx.vec_len, np.float64(dom.G ** 3)
    assert n == 3 * dom.G ** 3
    rs = np.random.RandomState(N + batch)
    x, y = _integers(rs, n * batch), _integers(rs, n * batch)
    want = np.array([np.float64(_int_dot(x[b * n:(b + 1) * n], y[b * n:(b + 1) * n])) / G3 for b in range(batch)])
    assert batch == 1 or len(set(want)) > 1                        # the members have sums of their own
    assert np.array_equal(np.atleast_1d(ctx.inner(x, y)), want)
    assert np.array_equal(np.atleast_1d(ctx.inner_dev(DeviceVector.from_numpy(x), DeviceVector.from_numpy(y))), want)
    # needles: x = e_i, y = 1 gives exactly 1 / G^3 — first, last and second-to-last element, both sides of every pass boundary
    idx = _kd_needles(n)
    ones = np.ones(n * batch)
    Y = DeviceVector.from_numpy(ones)
    x = np.zeros(n * batch)
    for j in range(len(idx)):
        hot = [b * n + idx[(j + b) % len(idx)] for b in range(batch)]      # another position in every member
        x[hot] = 1.
        assert np.all(np.atleast_1d(ctx.inner(x, ones)) == 1. / G3), (j, hot)
        assert np.all(np.atleast_1d(ctx.inner_dev(DeviceVector.from_numpy(x), Y)) == 1. / G3), (j, hot)
        x[hot] = 0.
    dom.drop_contexts()


# ---- KDyn energy (kd_energy: sum_k w |B^_k|^2, w = 1 on the kx = 0 plane and 2 off it) -----------------------------------------------------
def _energy_modes(kmax):
    """(component, (kx, ky, kz), amplitude): the grid field of each is amplitude * cos(k.x); every component is constant along its own axis,
    so k.B^ = 0 exactly.  On the kx = 0 plane (two coefficients of weight 1) and off it (one of weight 2), the mean, the truncation edge."""
    return [(0, (0, 0, 0), 2. ** -1), (0, (0, 2, 0), 1.), (0, (0, 3, -5), 2. ** -2),
            (1, (3, 0, 0), 2. ** -1), (1, (kmax, 0, -kmax), 2. ** -3), (1, (0, 0, kmax), 2. ** -2),
            (2, (1, -2, 0), 2. ** -4), (2, (0, 1, 0), 2. ** -5), (2, (kmax, kmax, 0), 2. ** -1)]


@pytest.mark.parametrize("N", [16, 22])          # G = 24 tuned; G = 33 run-time length, odd
@pytest.mark.parametrize("cost", ["Final", "Integrated"])
def test_kdyn_energy_of_a_power_of_two_spectrum(N, cost):
    """U = 0, no diffusion to rounding (Rm = 1e300: 1/dt +- k^2 / 2 Rm == 1/dt), dt a power of two: a step maps every mode onto itself
    exactly (the mean flips its sign), so J(Final) = -sum w |B^_0|^2 and J(Integrated) = -2 dt sum w |B^_0|^2 after one step, with the sum
    done by hand: a^2 for the mean, a^2 / 2 for every other cosine.  4 ulp: the transform of a single mode need not be bit-exact."""
    dom = kdyn.KDynDomain(N)
    G, dt = dom.G, 2. ** -7
    s = 2. * np.pi * np.arange(G) / G
    X, Y, Z = np.meshgrid(s, s, s, indexing="ij")
    B = np.zeros((3, G, G, G))
    E = 0.
    for comp, (kx, ky, kz), a in _energy_modes(dom.kmax):
        B[comp] += a * np.cos(kx * X + ky * Y + kz * Z)
        E += a * a if (kx, ky, kz) == (0, 0, 0) else 0.5 * a * a
    ctx = dom.context(1e300, dt, 1, cost)
    J = ctx.forward([B.reshape(-1), np.zeros(3 * G ** 3)])
    want = -E if cost == "Final" else -2. * dt * E
    print("kd_energy N=%d %s: J=%.17g want=%.17g  %.1f ulp" % (N, cost, J, want, _ulps(J, want)))
    assert _ulps(J, want) <= 4, (J, want)
    dom.drop_contexts()


# ---- SH23 Inner_Prod (sh23_inner_kernel: one workgroup per member, 256 lanes striding the 2 Npts grid) ------------------------------------
@pytest.mark.parametrize("Npts", [4, 21, 127, 128, 129, 1100])
@pytest.mark.parametrize("batch", [1, 5])
def test_sh23_inner_product_is_exact_on_integers(Npts, batch):
    dom = sh23.SH23Domain(Npts)
    ctx = dom.context(0.1, 1, batch=batch)
    G = dom.G
    rs = np.random.RandomState(Npts + batch)
    x, y = _integers(rs, G * batch), _integers(rs, G * batch)
    want = np.array([np.float64(_int_dot(x[b * G:(b + 1) * G], y[b * G:(b + 1) * G])) / np.float64(G) for b in range(batch)])
    assert batch == 1 or len(set(want)) > 1
    assert np.array_equal(np.atleast_1d(ctx.inner(x, y)), want)
    assert np.array_equal(np.atleast_1d(ctx.inner_dev(DeviceVector.from_numpy(x), DeviceVector.from_numpy(y))), want)
    ctx.close()


# ---- weighted inner products: needles against the oracle's weights ----------------------------------------------------------------------
def _needle_indices(n, seed):
    idx = {0, 1, n - 2, n - 1}
    for m in range(256, n, 256):
        idx.update(i for i in (m - 1, m, m + 1) if i < n)
    idx.update(int(i) for i in np.random.RandomState(seed).randint(0, n, 12))
    return sorted(idx)


def _check_needles(inner_dev, inner_ref, n, seed):
    """x = e_i, y = 1: the device must return the oracle's <e_i, 1> to 4 ulp for every needle; and <1, 1> the sum of the weights to 1e-14."""
    ones, x = np.ones(n), np.zeros(n)
    worst = 0.
    for i in _needle_indices(n, seed):
        x[i] = 1.
        got, want = inner_dev(x, ones), inner_ref(x, ones)
        x[i] = 0.
        worst = max(worst, _ulps(got, want))
        assert _ulps(got, want) <= 4, (i, got, want)
    got, want = inner_dev(ones, ones), inner_ref(ones, ones)
    assert abs(got - want) <= 1e-14 * abs(want), (got, want)
    return worst


@functools.lru_cache(maxsize=None)
def _shb_oracle(N, cnts):
    from oracle import shb23 as osh
    return (osh.SHB23CntsOracle if cnts else osh.SHB23Oracle)(N, dt=1e-2, N_ITERS=1)


@pytest.mark.parametrize("N", [8, 257, 1023, 1024])
def test_shb23_discrete_inner_product_needles(N):
    dom = shb23.SHBDomain(N)
    o = _shb_oracle(N, False)
    worst = _check_needles(lambda x, y: shb23.Inner_Prod_Discrete(x, y, dom), o.inner, N, N)
    print("shb23 discrete N=%d: worst needle %.1f ulp" % (N, worst))


# the Continuous formulation has Npts <= 512 modes on the 2 Npts grid: grid lengths 16, 514 and the largest, 1024 (an odd grid length,
# 257 or 1023, does not exist there)
@pytest.mark.parametrize("Npts", [8, 257, 512])
def test_shb23_continuous_inner_product_needles(Npts):
    """The quadrature weight of a needle is sum_k integ(T_k) T_k(z_i) over the even k < Npts, which cancels to 1e-3 of its terms near the
    end points of the interval.  The library builds the weights in extended precision on the host, and SHB23CntsOracle.inner transforms and
    sums in extended precision for the same reason: evaluated in double precision the sum is 242 (Npts 257) and 788 ulp (Npts 512) off at
    i = 0 — 9.865404570661007e-06 and 2.4883053910141824e-06 where 40 digits give 9.8654045706605958e-06 and 2.4883053910138483e-06,
    from which the device is 0.8 ulp away at most.  test_shb23_continuous_inner_product_needles_in_extended_precision sums the series
    itself, without a transform."""
    dom = shb23.SHBDomain(Npts, dealias=2)
    o = _shb_oracle(Npts, True)
    worst = _check_needles(lambda x, y: shb23.Inner_Prod_Cnts(x, y, dom), o.inner, 2 * Npts, Npts)
    print("shb23 continuous Npts=%d: worst needle %.1f ulp" % (Npts, worst))


@pytest.mark.parametrize("Npts", [8, 257, 512])
def test_shb23_continuous_inner_product_needles_in_extended_precision(Npts):
    """The same needles against <e_i, 1> = (1 / Lz) sum_{k even < Npts} integ(T_k) T_k(z_i) summed in np.longdouble, and <1, 1> = 1."""
    dom = shb23.SHBDomain(Npts, dealias=2)
    N, Lz = 2 * Npts, np.longdouble(dom.hypervolume)
    k = np.arange(0, Npts, 2).astype(np.longdouble)
    wk = Lz / (1 - k * k) * np.where(k == 0, np.longdouble(0.5), np.longdouble(1)) * 2 / N

    def inner_ref(x, y):
        i = np.flatnonzero(x * y)
        theta = 4 * np.arctan(np.longdouble(1)) * k[:, None] * (2 * i[None, :] + 1) / (2 * np.longdouble(N))
        return float(np.sum(wk[:, None] * np.cos(theta)) / Lz)

    worst = _check_needles(lambda x, y: shb23.Inner_Prod_Cnts(x, y, dom), inner_ref, N, Npts)
    print("shb23 continuous Npts=%d against extended precision: worst needle %.1f ulp" % (Npts, worst))


# pois_dot: 256 workgroups of 256 lanes, one element per lane and pass — 2 * 384 * 192 elements are 2.25 passes, and the multiples of 256
# +- 1 among the needles include both sides of every pass boundary
@pytest.mark.parametrize("Nx,Nz", [(24, 24), (30, 66), (96, 48), (384, 192)])
def test_poiseuille_discrete_inner_product_needles(Nx, Nz):
    from oracle.poiseuille import PoiseuilleOracle
    dom = pz.PoiseuilleDomain(Nx, Nz)
    o = PoiseuilleOracle(Nx, Nz)
    worst = _check_needles(lambda x, y: pz.Inner_Prod_Discrete(x, y, dom), o.inner, 2 * Nx * Nz, Nx + Nz)
    print("poiseuille %dx%d: worst needle %.1f ulp" % (Nx, Nz, worst))
    dom.drop_contexts()


# ---- DeviceVector algebra past the grid-stride caps (vec_axpby: 4096 workgroups x 256 lanes x 2 elements per pass) ---------------------------
@pytest.mark.parametrize("n", [2 * 4096 * 256 + 1537, 3 * 2 * 4096 * 256 + 2])      # odd with two passes (and the tail element); three passes and one pair
def test_algebra_rounds_like_numpy_past_one_pass(n):
    devvec_tests.test_algebra_rounds_like_numpy(n)


@pytest.mark.parametrize("with_y", [True, False])
def test_axpby_one_element_per_lane_past_one_pass(with_y):
    """smo_vec_axpby on a view at element offset 1 (8-byte aligned only: vec_axpby_scalar), n = 4096 * 256 + 777: two passes."""
    n = 4096 * 256 + 777
    rs = np.random.RandomState(8)
    x, y = rs.standard_normal(n + 1) * 10. ** rs.randint(-8, 8, n + 1), rs.standard_normal(n + 1)
    X, Y, O = DeviceVector.from_numpy(x), DeviceVector.from_numpy(y), DeviceVector.from_numpy(np.full(n + 1, 7.))
    a, b = 1.25, -0.3333333333333333
    L = _capi.lib()
    _capi._check(L.smo_vec_axpby(0, n, a, C.c_void_p(X.ptr + 8), b, C.c_void_p(Y.ptr + 8) if with_y else None, C.c_void_p(O.ptr + 8)))
    out = O.numpy()
    assert out[0] == 7.                                                        # the element before the view is not touched
    assert np.array_equal(out[1:], a * x[1:] + b * y[1:] if with_y else a * x[1:])
