"""The premises of tests/test_parameters_gpu.py, on the CPU oracle alone (no GPU): at the parameter sets of tests/parameter_cases.py every
physical parameter moves the oracle's answer by far more than the tolerance of the device comparison, so a kernel, an operator assembly or a
context key that ignored one of them could not pass there.  The oracle is unpinned against the reference at these parameters, so it is
held here to facts that do not come from its own closed forms: Pe = Re Pr is the only way Pr enters, the SHB23 tau operator solves its
boundary-value problem on a shifted interval, the gradients pass Taylor / central-difference checks, and KDyn refuses a box that is not 2 pi.

rel(a, b) = |a - b| / |b|.  Separations measured on the oracle (gradient at the parameter set against the gradient with ONE parameter set
back to its default, same input):

    Poiseuille, POIS_P against the default of ...     24 x 24 Discrete       16 x 16 Continuous     48 x 36 D    32 x 24 C
                                                      s = 0      s = 1       s = 0      s = 1       (smaller of s = 0, 1)
        Re       200 -> 500                           1.6e-1     1.4e-2      1.8e-1     5.2e-2      2.7e-2       7.9e-2
        Ri       2.0 -> 0.05                          4.8e-3     5.7e-3      4.6e-3     2.1e-2      6.4e-3       5.8e-3
        Prandtl  0.5 -> 1                             6.1e-5     8.5e-3      5.3e-5     1.6e-2      1.3e-4       1.1e-4
        Lx       7.0 -> 4 pi                          1.3e-1     1.8e-1      1.5e-1     6.6e-1      1.6e-1       2.1e-1
      b snapshot at step n: Re 2.8e-3 .. 1.1e-2, Prandtl 2.4e-3 .. 7.6e-3, Lx 1.8e-3 .. 6.0e-2
    Pe identity (X = 0, s = 1): J bit-equal and b to 6e-19 across (Re, Pr) = (500, 2), (1000, 1), (250, 4); (500, 1) differs by 1.0e-3 in J
      and 5.1e-4 (Discrete) / 5.6e-4 (Continuous) in b
    SH23, both adjoint types, Npts 64 and 54:         default a 4.5e-1 .. 2.4e0        default interval 3.8e-1 .. 3.8e0
    SHB23, both formulations, all sizes:              default a 1.8e-2 .. 6.4e-2       default interval 3.8e-2 .. 7.6e-2
    Taylor second-remainder slopes: SH23 within 5e-5 of 2, SHB23 (N = 128) within 6e-5
    Poiseuille <g, dX> against a central difference (eps = 1e-4): s = 0 4.4e-6 (24 x 24), 7e-10 (48 x 36); s = 1 1.1e-3, 2e-8
"""
import contextlib
import io

import numpy as np
import pytest

import parameter_cases as pc
from oracle import shb23 as osh
from oracle.sh23 import SH23Oracle
from parameter_cases import rel
from spheremanopt_amd.test_grad import taylor_table

RTOL = 1e-6                         # the device comparison's tolerance (test_parameters_gpu.py)
FLOOR_EVERY, FLOOR_ONE_COST = 10 * RTOL, 1e-3
FLOOR_B = 1e-4


def _taylor(X, dX, o, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return taylor_table([X], [dX], o.forward, o.adjoint, o.inner, **kw)


# ---- Poiseuille: sensitivity floor -------------------------------------------------------------------------------------------------------
def _pois_solve(Nx, Nz, s, continuous, **params):
    o = pc.pois_oracle(Nx, Nz, s, continuous, **params)
    X = pc.pois_input(Nx, Nz, continuous)
    J = o.forward([X])
    return J, o.adjoint([X])[0], o.stack[2, :, :, pc.POIS_N].copy()


@pytest.mark.parametrize("continuous,Nx,Nz", [(False,) + sz for sz in pc.POIS_DISCRETE_SIZES] + [(True,) + sz for sz in pc.POIS_CNTS_SIZES])
def test_poiseuille_every_parameter_moves_the_gradient(continuous, Nx, Nz):
    """A condition on the parameter set, not a measurement: with one parameter back at its default the gradient moves by >= 10 RTOL for
    both costs and by >= 1e-3 for at least one; the last b snapshot moves by >= 1e-4 for Re, Prandtl and Lx."""
    base = {s: _pois_solve(Nx, Nz, s, continuous) for s in (0, 1)}
    for p in ("Re", "Ri", "Prandtl", "Lx"):
        assert pc.POIS_P[p] != pc.POIS_DEFAULT[p]
        seps = []
        for s in (0, 1):
            J, g, b = _pois_solve(Nx, Nz, s, continuous, **{p: pc.POIS_DEFAULT[p]})
            seps.append(rel(g, base[s][1]))
            print("%s %d x %d  s = %d  %-8s gradient %.2e  b_n %.2e" % ("C" if continuous else "D", Nx, Nz, s, p, seps[-1], rel(b, base[s][2])))
            assert seps[-1] >= FLOOR_EVERY, (p, s, seps[-1])
            if p != "Ri":
                assert rel(b, base[s][2]) >= FLOOR_B, (p, s, rel(b, base[s][2]))
        assert max(seps) >= FLOOR_ONE_COST, (p, seps)


# ---- Poiseuille: Pr enters through Pe = Re Pr and in no other way ---------------------------------------------------------------------
@pytest.mark.parametrize("continuous,Nx,Nz", [(False, 24, 24), (True, 16, 16)])
def test_poiseuille_pe_identity(continuous, Nx, Nz):
    """X = 0: the velocity stays zero, b diffuses with 1 / Pe, and the mix-norm of b(T) is the cost — Re alone no longer matters.  Equal
    Re Pr must give the same J and b stack (1e-11); Re Pr = 500 must not."""
    def solve(Re, Pr):
        o = pc.pois_oracle(Nx, Nz, 1, continuous, Re=Re, Prandtl=Pr)
        J = o.forward([np.zeros(2 * (o.Gx * o.Gz if continuous else Nx * Nz))])
        assert np.abs(o.stack[:2, :, :, :pc.POIS_N]).max() < 1e-14               # u, w snapshots (slot N of the Discrete stack holds grad psi)
        return J, o.stack[2].copy()

    J0, b0 = solve(*pc.POIS_PE_PAIRS[0])
    for Re, Pr in pc.POIS_PE_PAIRS[1:]:
        J, b = solve(Re, Pr)
        print("Re %g Pr %g: J %.2e  b %.2e" % (Re, Pr, abs(J - J0) / abs(J0), rel(b, b0)))
        assert abs(J - J0) <= 1e-11 * abs(J0) and rel(b, b0) <= 1e-11, (Re, Pr)
    J, b = solve(*pc.POIS_PE_OTHER)
    print("Re %g Pr %g: J %.2e  b %.2e" % (pc.POIS_PE_OTHER + (abs(J - J0) / abs(J0), rel(b, b0))))
    assert abs(J - J0) > 1e-4 * abs(J0) and rel(b, b0) > 1e-4


# ---- Poiseuille: the Discrete gradient at POIS_P against a central difference -----------------------------------------------------------
@pytest.mark.parametrize("Nx,Nz", pc.POIS_DISCRETE_SIZES)
@pytest.mark.parametrize("s,bound", [(0, 1e-4), (1, 2e-3)])
def test_poiseuille_gradient_against_central_difference(Nx, Nz, s, bound):
    o = pc.pois_oracle(Nx, Nz, s)
    X, dX = pc.pois_input(Nx, Nz, seed=42), pc.pois_input(Nx, Nz, seed=7)
    o.forward([X])
    d = o.inner(o.adjoint([X])[0], dX)
    eps = 1e-4
    fd = (o.forward([X + eps * dX]) - o.forward([X - eps * dX])) / (2. * eps)
    print("%d x %d s = %d: %.2e" % (Nx, Nz, s, abs(d - fd) / abs(fd)))
    assert abs(d - fd) < bound * abs(fd), (d, fd)


# ---- SH23 --------------------------------------------------------------------------------------------------------------------------------
def _sh_grad(Npts, interval, a, adj):
    o = SH23Oracle(Npts, interval=interval, dt=pc.SH23_DT, N_ITERS=pc.SH23_N, a=a)
    o.forward([pc.sh23_input(Npts)])
    return o.adjoint(None, adj)[0]


@pytest.mark.parametrize("Npts", pc.SH23_NPTS)
@pytest.mark.parametrize("interval,a", pc.SH23_CASES)
def test_sh23_interval_and_a_move_the_gradient(Npts, interval, a):
    for adj in ("Discrete", "Continuous"):
        g = _sh_grad(Npts, interval, a, adj)
        sa, si = rel(_sh_grad(Npts, interval, pc.SH23_DEFAULT[1], adj), g), rel(_sh_grad(Npts, pc.SH23_DEFAULT[0], a, adj), g)
        print("sh23 %d %s a = %g %s: default a %.2e  default interval %.2e" % (Npts, interval, a, adj, sa, si))
        assert sa >= FLOOR_ONE_COST and si >= FLOOR_ONE_COST, (adj, sa, si)


@pytest.mark.parametrize("Npts", pc.SH23_NPTS)
@pytest.mark.parametrize("interval,a", pc.SH23_CASES)
def test_sh23_taylor(Npts, interval, a):
    o = SH23Oracle(Npts, interval=interval, dt=pc.SH23_DT, N_ITERS=pc.SH23_N, a=a)
    AA = _taylor(pc.sh23_input(Npts, 42), pc.sh23_input(Npts, 7), o, epsilon=1e-3)
    assert np.all(np.abs(AA[4, :4] - 2.) < 5e-3), AA


def test_sh23_known_answer_with_L_and_a():
    """The closed form of the device test (parameter_cases.sh23_growth) on the oracle: the factor is not the oracle's own 1 / A."""
    dt, n, eps, m = pc.SH23_DT, pc.SH23_N, 1e-9, 5
    for interval, a in pc.SH23_CASES:
        o = SH23Oracle(64, interval=interval, dt=dt, N_ITERS=n, a=a)
        X = eps * np.cos(2. * np.pi * m * np.arange(o.G) / o.G)
        r = pc.sh23_growth(interval[1] - interval[0], a, m, dt)
        expect = -dt * 0.5 * eps ** 2 * sum(r ** (2 * i) for i in range(n + 1))
        assert abs(o.forward([X]) - expect) < 1e-7 * abs(expect)


# ---- SHB23 -------------------------------------------------------------------------------------------------------------------------------
def _shb_grad(N, n, interval, a, continuous, X):
    o = pc.shb23_oracle(N, n, interval, a, continuous)
    o.forward([X])
    return o.adjoint(None)[0]


@pytest.mark.parametrize("continuous,N,n", [(False,) + sz for sz in pc.SHB23_DISCRETE_SIZES] + [(True,) + sz for sz in pc.SHB23_CNTS_SIZES])
@pytest.mark.parametrize("interval,a", pc.SHB23_CASES)
def test_shb23_interval_and_a_move_the_gradient(continuous, N, n, interval, a):
    X = pc.shb23_input(N, interval, a, continuous)
    g = _shb_grad(N, n, interval, a, continuous, X)
    sa = rel(_shb_grad(N, n, interval, pc.SHB23_DEFAULT[1], continuous, X), g)
    si = rel(_shb_grad(N, n, pc.SHB23_DEFAULT[0], a, continuous, X), g)
    print("shb23 %s N = %d %s a = %g: default a %.2e  default interval %.2e" % ("C" if continuous else "D", N, interval, a, sa, si))
    assert sa >= FLOOR_ONE_COST and si >= FLOOR_ONE_COST, (sa, si)


@pytest.mark.parametrize("interval,a", pc.SHB23_CASES)
def test_shb23_taylor(interval, a):
    """N = 128 as in test_oracle.test_taylor_shb23 (below that the reference's missing Z^T in NLtermAdj shows in the slopes)."""
    N, n = 128, 100
    o = pc.shb23_oracle(N, n, interval, a)
    AA = _taylor(pc.shb23_input(N, interval, a, seed=42), pc.shb23_input(N, interval, a, seed=7), o, epsilon=1e-3)
    assert np.all(np.abs(AA[4, :4] - 2.) < 5e-3), AA


@pytest.mark.parametrize("interval,a", pc.SHB23_CASES)
def test_shb_tau_operator_solves_the_bvp_on_another_interval(interval, a):
    """test_oracle.test_shb_tau_operator_solves_the_bvp with the interval and a as arguments: S r must be the spectrally accurate solution of
    (1/dt + 1 - a + 2 d2 + d4) u = r with u'(x0) = u'''(x0) = 0, u(x1) = u''(x1) = 0.  The right-hand side is recentred on the midpoint and
    its width scaled by (x1 - x0) / 40; the evaluation points lie in the middle three quarters.  Same tolerances."""
    from numpy.polynomial import chebyshev as C
    dt = pc.SHB23_DT
    x0, x1 = interval
    c, w = 0.5 * (x0 + x1), (x1 - x0) / 40.
    rhs = lambda z: np.exp(-((z - c) / (4. * w)) ** 2) * np.cos((z - c) / w)      # noqa: E731
    zz = c + w * np.linspace(-15, 15, 7)
    assert zz[0] >= c - 0.375 * (x1 - x0) and zz[-1] <= c + 0.375 * (x1 - x0)
    sols = []
    for N in (64, 96):
        S = osh.tau_operator(N, dt, a, interval)
        u = S @ osh.transform(rhs(osh.gauss_grid(N, interval)))
        p = C.Chebyshev(u, domain=[x0, x1])
        tol = 1e-3 if N == 64 else 1e-9
        assert abs(p(x1)) < 1e-14 and abs(p.deriv(2)(x1)) < tol
        assert abs(p.deriv(1)(x0)) < tol and abs(p.deriv(3)(x0)) < tol
        res = (1 / dt + 1 - a) * p(zz) + 2 * p.deriv(2)(zz) + p.deriv(4)(zz) - rhs(zz)
        assert np.abs(res).max() < (1e-7 if N == 64 else 1e-12)
        sols.append(p(zz))
    assert np.abs(sols[0] - sols[1]).max() < 1e-9


# ---- KDyn: a box that is not 2 pi is refused before the library is touched ---------------------------------------------------------------
def test_kdyn_domains_refuse_another_box_length(monkeypatch):
    from spheremanopt_amd import _capi, kdyn, kdyn_slab

    def no_library(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_capi, "lib", no_library)
    for cls in (kdyn.KDynDomain, kdyn_slab.SlabDomain):
        with pytest.raises(ValueError, match="2 pi"):
            cls(24, X=pc.KDYN_BAD_INTERVAL)
        for X in pc.KDYN_GOOD_INTERVALS:
            assert cls(24, X=X).G == 36
    with pytest.raises(ValueError, match="2 pi"):
        kdyn.Generate_IC(24, X=pc.KDYN_BAD_INTERVAL)
