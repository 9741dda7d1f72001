"""The premises of tests/test_kdyn_exact_gpu.py, pinned on the CPU oracle (tests/exact_ops.py states them): the Discrete adjoint is the EXACT
gradient of a cost that is a polynomial along U + t d, read off by a central stencil with exact weights; with a uniform flow the time step
is a 3 x 3 matrix per mode.  No GPU.

Statement A is asserted with the bound the GPU test uses (exact_ops.needle_defect: JTOL = 1e-12 on every J of the stencil, GTOL = 1e-11 on
|g| |d|), and that bound must stay below SHARE = 1e-8 of |g| |d|.  Observed on the oracle, as shares of |g| |d|: defect <= 2.7e-16 for gB
and <= 1.2e-14 for gU at dt = 1e-2 (9.8e-14 at dt = 1e-3), bound <= 1.3e-10 at dt = 1e-2 and 1.3e-9 at dt = 1e-3.  A white-noise or a
constant direction misses by more than 1e-4 of |g| |d|, as it must.
Statement B: the oracle's worst per-element defect against the longdouble closed form is 9.6e-16 of max |S_0| (Npts 8, 10, 16; 9 steps).
The sensitivity tests show a 1e-8 error, planted in one Fourier coefficient, rejected by these bounds and accepted by the norm tolerances
of the oracle comparisons (1e-6 for gradients, 1e-9 for snapshots).
"""
from fractions import Fraction

import numpy as np
import pytest

from exact_ops import (GTOL, JTOL, ORACLE_UNIFORM_DEFECT, RTOL, SHARE, UNIFORM_FLOW, UNIFORM_TOL, boundary_needles, few_needles, inner, mode_index,
                       needle_defect, needle_wavenumbers, perp_amplitude, plane_wave, stencil_weights, uniform_flow_steps, unit_needle,
                       wavenumbers)
from oracle.kdyn import KDynOracle, synthetic_field
from symmetry_ops import kd_cheap_field, kd_dirty_fields, rel

RM = 1.3
SNAP_RTOL = 1e-9                          # the norm tolerance the snapshots are compared with elsewhere


# ---- the helpers themselves ----------------------------------------------------------------------------------------------------------
def test_stencil_weights_satisfy_the_moment_conditions():
    assert stencil_weights(1) == [0.5]
    assert stencil_weights(2) == [2. / 3., -1. / 12.]
    assert stencil_weights(3) == [3. / 4., -3. / 20., 1. / 60.]
    for n in range(1, 7):
        w = [Fraction(v) for v in stencil_weights(n)]           # the floats, exactly
        for i in range(n):
            moment = sum(wj * Fraction(j) ** (2 * i + 1) for j, wj in enumerate(w, 1))
            size = sum(abs(wj) * Fraction(j) ** (2 * i + 1) for j, wj in enumerate(w, 1))
            assert abs(moment - Fraction(1 if i == 0 else 0, 2)) <= Fraction(1, 2 ** 52) * size, (n, i)


@pytest.mark.parametrize("kmax", [2, 3, 4, 5, 10, 36, 63, 127])
def test_needle_wavenumbers(kmax):
    ks = needle_wavenumbers(kmax)
    assert len(ks) == len(set(ks)) == 10 and (0, 0, 0) not in ks
    assert all(abs(c) <= kmax for k in ks for c in k)
    assert any(k[1] < 0 for k in ks) and any(k[2] < 0 for k in ks)
    assert any(max(abs(c) for c in k) < kmax for k in ks[8:])               # the seeded ones are interior
    for sub in (boundary_needles(kmax), few_needles(kmax)):
        assert set(sub) <= set(ks)
    assert ks == needle_wavenumbers(kmax)


@pytest.mark.parametrize("N", [6, 8, 10])
def test_a_needle_is_one_fourier_coefficient(N):
    """unit_needle: <d, d> = 1, solenoidal, and every coefficient but the one at k (and its mirror image on kx = 0) is zero."""
    o = KDynOracle(N)
    rs = np.random.RandomState(1)
    for k in needle_wavenumbers(o.kmax):
        d = unit_needle(o.G, k, rs)
        assert abs(inner(d, d, o.G) - 1.) < 1e-13
        C = o.vec_to_coeff(d)
        assert np.abs(o.kdot(C)).max() < 1e-14
        idx = mode_index(k, o.kmax)
        assert np.abs(C[(slice(None),) + idx]).max() > 0.3
        C[(slice(None),) + idx] = 0.
        if k[0] == 0:
            C[(slice(None),) + mode_index((0, -k[1], -k[2]), o.kmax)] = 0.
        assert np.abs(C).max() < 1e-14, k
        assert rel(o.coeff_to_vec(o.vec_to_coeff(d)), d) < 1e-14             # band-limited: the truncation keeps all of it
    a = perp_amplitude((3, -2, 1), rs)
    assert abs(a @ np.array([3., -2., 1.])) < 1e-15 and abs(np.linalg.norm(a) - 1.) < 1e-15
    x = 2. * np.pi * np.arange(o.G) / o.G
    X, Y, Z = np.meshgrid(x, x, x, indexing='ij')
    assert np.abs(plane_wave(o.G, (1, -2, 2), (1., 2., 3.), 0.3).reshape(3, -1)[1] - 2. * np.cos(X - 2. * Y + 2. * Z + 0.3).ravel()).max() < 1e-14


# ---- statement A ---------------------------------------------------------------------------------------------------------------------
_A_CASES = [(N, 2, 1e-2, c) for N in (8, 10, 12) for c in ("Final", "Integrated")] + [(8, 3, 1e-2, c) for c in ("Final", "Integrated")] + \
           [(8, 2, 1e-3, "Integrated")]             # the last: the dt and the inputs of the GPU test above G = 96


@pytest.fixture(scope="module", params=_A_CASES, ids=lambda p: "N%d-n%d-dt%g-%s" % p)
def base(request):
    N, n, dt, cost = request.param
    o = KDynOracle(N, Rm=RM, dt=dt, N_ITERS=n, Cost_function=cost)
    if dt == 1e-2:
        B, U = kd_dirty_fields(o.G, synthetic_field)
    else:
        B, U = kd_cheap_field(o.G, 9), kd_cheap_field(o.G, 10, mean=0.)
    o.forward([B, U])
    gB, gU = o.adjoint([B, U], "Discrete")
    return o, n, B, U, gB, gU


def _J_in_B(o, B, U, d):
    return [o.forward([B + d, U])], [o.forward([B - d, U])]


def _J_in_U(o, n, B, U, d):
    return [o.forward([B, U + j * d]) for j in range(1, n + 1)], [o.forward([B, U - j * d]) for j in range(1, n + 1)]


def test_discrete_adjoint_is_the_exact_gradient(base):
    o, n, B, U, gB, gU = base
    rs = np.random.RandomState(3)
    dirs = [unit_needle(o.G, k, rs) for k in needle_wavenumbers(o.kmax)] + [gU / np.sqrt(inner(gU, gU, o.G))]
    for d in dirs:
        for g, w, (Jp, Jm) in ((gB, stencil_weights(1), _J_in_B(o, B, U, d)), (gU, stencil_weights(n), _J_in_U(o, n, B, U, d))):
            defect, bound, gd = needle_defect(g, d, w, Jp, Jm, o.G)
            assert defect <= bound, (defect / gd, bound / gd)
            assert bound < SHARE * gd, bound / gd


def test_the_plain_central_difference_is_not_exact(base):
    """Why the weights matter: the 2-point difference of the same J does not pass the bound (off by 2e-8 of |g| |d| at dt = 1e-3, by 1e-5 and
    more at dt = 1e-2)."""
    o, n, B, U, gB, gU = base
    d = unit_needle(o.G, (1, 0, 0), np.random.RandomState(3))
    Jp, Jm = _J_in_U(o, n, B, U, d)
    defect, bound, gd = needle_defect(gU, d, [0.5], Jp[:1], Jm[:1], o.G)
    assert defect > 10. * bound, (defect / gd, bound / gd)


def test_directions_outside_the_adjoints_range_break_the_identity(base):
    """White noise (not solenoidal, not band-limited) and a constant (the k = 0 mode, which the constraint row flips): the identity fails,
    by design."""
    o, n, B, U, gB, gU = base
    noise = np.random.RandomState(4).standard_normal(B.size)
    const = np.repeat(np.array([0.6, -0.5, 0.4]), o.G ** 3)
    for d in (noise / np.sqrt(inner(noise, noise, o.G)), const):
        for g, w, (Jp, Jm) in ((gB, stencil_weights(1), _J_in_B(o, B, U, d)), (gU, stencil_weights(n), _J_in_U(o, n, B, U, d))):
            defect, bound, gd = needle_defect(g, d, w, Jp, Jm, o.G)
            assert defect > 1e-4 * gd > 100. * bound, (defect / gd, bound / gd)


def test_a_planted_error_of_1e_8_in_one_coefficient(base):
    """g + 1e-8 |g| d for a unit needle d: the needle's assertion rejects it; the norm comparison at RTOL accepts it."""
    o, n, B, U, gB, gU = base
    rs = np.random.RandomState(5)
    for k in few_needles(o.kmax):
        d = unit_needle(o.G, k, rs)
        for g, w, (Jp, Jm) in ((gB, stencil_weights(1), _J_in_B(o, B, U, d)), (gU, stencil_weights(n), _J_in_U(o, n, B, U, d))):
            bad = g + 1e-8 * np.sqrt(inner(g, g, o.G)) * d
            defect, bound, gd = needle_defect(bad, d, w, Jp, Jm, o.G)
            assert defect > bound, (k, defect / gd, bound / gd)
            assert rel(bad, g) < RTOL
            defect, bound, gd = needle_defect(g, d, w, Jp, Jm, o.G)
            assert defect <= bound


# ---- statement B ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[8, 10, 16], ids=lambda N: "N%d" % N)
def uniform(request):
    N, n, dt = request.param, 9, 1e-2
    o = KDynOracle(N, Rm=RM, dt=dt, N_ITERS=n)
    o.forward([kd_cheap_field(o.G, 9), np.repeat(np.array(UNIFORM_FLOW), o.G ** 3)])
    S = np.moveaxis(o.stack, -1, 0).copy()
    K = wavenumbers(N)
    assert np.array_equal(K, o.K)
    return o, S, [E for E in uniform_flow_steps(S[0], K, UNIFORM_FLOW, RM, dt, n)]


def _uniform_defect(S, expect):
    return max(float(np.abs(S[i] - E).max()) for i, E in enumerate(expect, 1)) / float(np.abs(S[0]).max())


def test_uniform_flow_every_mode(uniform):
    """Every element of every snapshot against the per-mode closed form.  The recorded figure is the oracle's worst; the device gets 32 times
    it, the oracle itself must stay within twice it."""
    o, S, expect = uniform
    assert UNIFORM_TOL == 32. * ORACLE_UNIFORM_DEFECT <= 1e-12
    defect = _uniform_defect(S, expect)
    assert defect <= 2. * ORACLE_UNIFORM_DEFECT, defect
    kB = (o.K * S[0]).sum(0)
    assert np.abs(kB).max() > 0.01 and np.abs(S[0][:, 0, 0, 0]).max() > 0.01       # B0 is not solenoidal and has a mean: both rows are exercised


def test_one_mode_of_one_snapshot_scaled_by_1e_8(uniform):
    """The per-element bound rejects it, the norm comparison of the snapshots accepts it."""
    o, S, expect = uniform
    bad = S.copy()
    idx = (4, 1) + mode_index((1, -2, o.kmax), o.kmax)               # the y component of snapshot 4, a mode on the truncation boundary
    bad[idx] *= 1. + 1e-8
    assert _uniform_defect(bad, expect) > UNIFORM_TOL
    assert _uniform_defect(S, expect) <= UNIFORM_TOL
    assert rel(bad[4], S[4]) < SNAP_RTOL
