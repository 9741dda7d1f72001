"""The premises of tests/test_symmetry_gpu.py, pinned on the CPU oracle: every identity demanded of the kernels there is one the oracle
itself satisfies to rounding, so an edit of the oracle cannot silently invalidate those tests.  No GPU.

Bound: 1e-13 relative — two orders above the defects the oracle shows (J <= 2e-16, gradients <= 2.5e-15; the quadratic-form identities of
KDyn <= 8e-15 of |J|).  Power-of-two scaling of B0 is exact in floating point and compared with ==.
"""
import numpy as np
import pytest

from oracle.kdyn import KDynOracle, synthetic_field
from oracle.poiseuille import PoiseuilleCntsOracle, PoiseuilleOracle, synthetic_ic, synthetic_ic_cnts
from oracle.sh23 import SH23Oracle
from oracle.sh23 import synthetic_ic as sh_ic
from symmetry_ops import kd_dirty_fields, kd_perm, kd_roll, pz_roll, rel, sh_reflect, sh_roll

TOL = 1e-13


def _kd_solve(o, B, U, adj):
    J = o.forward([B, U])
    gB, gU = o.adjoint([B, U], adj)
    return J, gB, gU


@pytest.fixture(scope="module", params=[(8, "Integrated", "Discrete"), (10, "Final", "Continuous")], ids=lambda p: "N%d-%s-%s" % p)
def kd_base(request):
    N, cost, adj = request.param
    o = KDynOracle(N, Rm=1.3, dt=1e-2, N_ITERS=2, Cost_function=cost)
    B, U = kd_dirty_fields(o.G, synthetic_field)
    return o, adj, B, U, _kd_solve(o, B, U, adj)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_kdyn_translation(kd_base, axis):
    o, adj, B, U, (J, gB, gU) = kd_base
    G = o.G
    for s in (1, 3, G - 1):
        sh = tuple(s if a == axis else 0 for a in range(3))
        J1, gB1, gU1 = _kd_solve(o, kd_roll(B, G, sh), kd_roll(U, G, sh), adj)
        assert abs(J1 - J) <= TOL * abs(J), (s, J1, J)
        assert rel(gB1, kd_roll(gB, G, sh)) < TOL and rel(gU1, kd_roll(gU, G, sh)) < TOL, s


def test_kdyn_cyclic_relabelling_of_the_axes(kd_base):
    o, adj, B, U, (J, gB, gU) = kd_base
    G = o.G
    J1, gB1, gU1 = _kd_solve(o, kd_perm(B, G), kd_perm(U, G), adj)
    assert abs(J1 - J) <= TOL * abs(J), (J1, J)
    assert rel(gB1, kd_perm(gB, G)) < TOL and rel(gU1, kd_perm(gU, G)) < TOL


def test_kdyn_power_of_two_scaling_is_exact(kd_base):
    o, adj, B, U, (J, gB, gU) = kd_base
    J2, gB2, gU2 = _kd_solve(o, 2. * B, U, adj)
    assert J2 == 4. * J
    assert np.array_equal(gB2, 2. * gB) and np.array_equal(gU2, 4. * gU)


def test_kdyn_cost_is_a_quadratic_form_in_B0(kd_base):
    """Parallelogram law with a dirty direction, and <gB, d> = (J(B+d) - J(B-d)) / 2 for the DISCRETE adjoint with a solenoidal direction (the
    adjoint projects: a non-solenoidal d does not satisfy it, by design)."""
    o, adj, B, U, (J, gB, gU) = kd_base
    G = o.G
    d = 0.3 * np.random.RandomState(11).standard_normal(B.size) + 0.02
    Jp, Jm, Jd = o.forward([B + d, U]), o.forward([B - d, U]), o.forward([d, U])
    assert abs(0.5 * (Jp + Jm) - J - Jd) <= TOL * (abs(Jp) + abs(Jm) + abs(J) + abs(Jd))
    o.forward([B, U])
    gBd = o.adjoint([B, U], "Discrete")[0]
    for d in (synthetic_field(G, 5), 8. * synthetic_field(G, 6)):
        Jp, Jm = o.forward([B + d, U]), o.forward([B - d, U])
        lhs = o.inner(gBd, d)
        assert abs(lhs - 0.5 * (Jp - Jm)) <= TOL * abs(lhs), (lhs, 0.5 * (Jp - Jm))


@pytest.mark.parametrize("Npts", [16, 21])
@pytest.mark.parametrize("adj", ["Discrete", "Continuous"])
def test_sh23_translation_and_reflection(Npts, adj):
    o = SH23Oracle(Npts, dt=0.1, N_ITERS=20)
    X = sh_ic(o.G, 42, 0.0725) + 0.05 * np.random.RandomState(3).standard_normal(o.G) + 0.01      # full spectrum, non-zero mean
    J = o.forward([X]); g = o.adjoint([X], adj)[0]
    for name, op in (("roll 1", lambda v: sh_roll(v, 1)), ("roll 7", lambda v: sh_roll(v, 7)), ("reflection", sh_reflect)):
        J1 = o.forward([op(X)]); g1 = o.adjoint([op(X)], adj)[0]
        assert abs(J1 - J) <= TOL * abs(J), (name, J1, J)
        assert rel(g1, op(g)) < TOL, (name, rel(g1, op(g)))


@pytest.mark.parametrize("Nx,Nz,s", [(24, 24, 0), (30, 18, 1)])
def test_poiseuille_discrete_translation_along_x(Nx, Nz, s):
    o = PoiseuilleOracle(Nx, Nz, dt=5e-3, N_ITERS=5, s=s, delta=0.3)
    X = synthetic_ic(o, 42)
    J = o.forward([X]); g = o.adjoint([X])[0]
    for sh in (1, 5):
        Xr = pz_roll(X, (Nx, Nz), sh)
        J1 = o.forward([Xr]); g1 = o.adjoint([Xr])[0]
        assert abs(J1 - J) <= TOL * abs(J), (sh, J1, J)
        assert rel(g1, pz_roll(g, (Nx, Nz), sh)) < TOL, (sh, rel(g1, pz_roll(g, (Nx, Nz), sh)))


@pytest.mark.parametrize("Nx,Nz,s", [(16, 16, 0), (16, 16, 1)])
def test_poiseuille_continuous_translation_along_x(Nx, Nz, s):
    """The Continuous formulation on its 3/2 grid: vectors are (3 Nx / 2, 3 Nz / 2) grids."""
    o = PoiseuilleCntsOracle(Nx, Nz, dt=5e-3, N_ITERS=5, s=s, delta=0.3)
    X = (10. if s == 1 else 1.) * synthetic_ic_cnts(o, 42)
    gs = (o.Gx, o.Gz)
    J = o.forward([X]); g = o.adjoint([X])[0]
    for sh in (1, 5):
        Xr = pz_roll(X, gs, sh)
        J1 = o.forward([Xr]); g1 = o.adjoint([Xr])[0]
        assert abs(J1 - J) <= TOL * abs(J), (sh, J1, J)
        assert rel(g1, pz_roll(g, gs, sh)) < TOL, (sh, rel(g1, pz_roll(g, gs, sh)))
