"""Oracle-free checks of the device paths: exact symmetries of the discrete equations (tests/symmetry_ops.py; pinned on the CPU oracle
by test_symmetry_oracle_cpu.py), exact power-of-two scaling, and the quadratic-form identities of the KDyn cost.  Each compares one device
solve with another device solve of transformed inputs, so nothing here depends on oracle/ — and every tuned KDyn size, the large ones the
oracle is too slow for included, sees full-spectrum data.

rel(a, b) = |a - b| / |b|.  Tolerances are the project's figures for "same arithmetic, other summation order"
(test_runtime_length_kernels_match_the_tuned_ones, the SH23 and Poiseuille path-against-path tests): J 1e-12 relative and gradients
rel 1e-11 for KDyn and SH23; 1e-11 for both with Poiseuille.  Scaling of B0 by 2 and a repeated solve are compared with ==.

Largest defects observed on an MI355X (J relative / gradients rel; a run with -s prints the table at its end):
    KDyn  translation, Npts 6..128:                   J 2.6e-16   gradients 1.4e-15
    KDyn  relabelling, Npts 6..128:                   J 3.4e-15   gradients 1.5e-15
    KDyn  large sizes, translation:                   J 2.9e-16   gradients 1.3e-15
    KDyn  large sizes, relabelling:                   J 4.5e-15   gradients 1.3e-15
    KDyn  five symmetric members of one batch:        J 0         gradients 7.1e-16
    KDyn  parallelogram: 5.1e-16 of the sum of the |J|;  <gB,d>: 2.8e-5 of its bound
    SH23  translation and reflection:                 J 4.6e-16   gradients 1.2e-15
    Pois  translation along x, Discrete:              J 3.7e-16   gradients 1.0e-15
    Pois  translation along x, Continuous:            J 1.9e-16   gradients 1.3e-15
Scaling by 2 and the repeated solve were bit-exact at every size.
"""
import numpy as np
import pytest

from spheremanopt_amd import kdyn, poiseuille as pz, sh23
from symmetry_ops import kd_cheap_field, kd_dirty_fields, kd_perm, kd_roll, pz_roll, rel, sh_reflect, sh_roll

pytestmark = pytest.mark.gpu
JTOL, GTOL = 1e-12, 1e-11
PTOL = 1e-11
RM, NSTEPS = 1.3, 2

_WORST = {}


def _note(family, J_defect, g_defect):
    w = _WORST.setdefault(family, [0., 0.])
    w[0], w[1] = max(w[0], J_defect), max(w[1], g_defect)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    _drop_base()
    for fam in sorted(_WORST):
        print("\nlargest defect  %-28s J %.2e   gradients %.2e" % (fam, _WORST[fam][0], _WORST[fam][1]), end="")
    print()


# ---- KDyn ----------------------------------------------------------------------------------------------------------------------------
_TUNED = [8, 12, 16, 20, 24, 28, 32, 36, 40, 48, 56, 60, 64, 72, 80, 96, 100, 112, 120, 128]      # include/smo.h, up to 128
_ANY = [6, 10, 22, 44, 74, 106]                       # run-time-length kernels: odd G, prime factors 11, 37, 53
_SMALL = sorted(_TUNED + _ANY)
_LARGE = [144, 160, 192, 200, 224, 240, 320, 310, 256]      # G = 216 .. 480; 310: run-time length (G = 465, odd); 256: the north-star grid
_ALL4 = [(c, a) for c in ("Final", "Integrated") for a in ("Discrete", "Continuous")]
_COMBO = {N: _ALL4[i % 4] for i, N in enumerate(_SMALL + _LARGE)}      # the four cost / adjoint combinations alternate across the sizes


def _kd_inputs(G):
    """Dirty fields (not solenoidal, non-zero mean, full spectrum); above G = 96 without host FFTs."""
    if G <= 96:
        return kd_dirty_fields(G, kdyn.synthetic_field)
    return kd_cheap_field(G, 9), kd_cheap_field(G, 10, mean=0.)


def _kd_dt(G):
    return 1e-2 if G <= 96 else 1e-3


_BASE = {}


def _drop_base():
    for v in _BASE.values():
        v["dom"].drop_contexts()
    _BASE.clear()


def _kd_base(N):
    """The base solve of a size, made once and shared by that size's checks; one size at a time (2 x 2.65 GB of inputs at G = 480)."""
    if N not in _BASE:
        _drop_base()
        dom = kdyn.KDynDomain(N)
        cost, adj = _COMBO[N]
        ctx = dom.context(RM, _kd_dt(dom.G), NSTEPS, cost)
        B, U = _kd_inputs(dom.G)
        J = ctx.forward([B, U])
        gB, gU = ctx.adjoint(None, adj)
        _BASE[N] = dict(dom=dom, ctx=ctx, adj=adj, B=B, U=U, J=J, gB=gB, gU=gU)
    return _BASE[N]


def _kd_check_image(b, op, family):
    """Solve op(inputs): J must equal the base J and the gradients op(base gradients)."""
    ctx = b["ctx"]
    J1 = ctx.forward([op(b["B"]), op(b["U"])])
    gB1, gU1 = ctx.adjoint(None, b["adj"])
    dJ = abs(J1 - b["J"]) / abs(b["J"])
    dB, dU = rel(gB1, op(b["gB"])), rel(gU1, op(b["gU"]))
    _note(family, dJ, max(dB, dU))
    assert dJ <= JTOL, (J1, b["J"])
    assert dB < GTOL and dU < GTOL, (dB, dU)


def _kd_check_scaling(b):
    """J is a quadratic form in B0: doubling B0 is exact in floating point.  Then the base solve again on the same context: bit for bit the
    first result (no stale running sum, no read of memory the solve did not write)."""
    ctx = b["ctx"]
    J2 = ctx.forward([2. * b["B"], b["U"]])
    gB2, gU2 = ctx.adjoint(None, b["adj"])
    assert J2 == 4. * b["J"], (J2, b["J"])
    assert np.array_equal(gB2, 2. * b["gB"]) and np.array_equal(gU2, 4. * b["gU"])
    del gB2, gU2
    J3 = ctx.forward([b["B"], b["U"]])
    gB3, gU3 = ctx.adjoint(None, b["adj"])
    assert J3 == b["J"], (J3, b["J"])
    assert np.array_equal(gB3, b["gB"]) and np.array_equal(gU3, b["gU"])


_SMALL_CHECKS = ("x", "y", "z", "perm", "scale")


@pytest.mark.parametrize("N,check", [(N, c) for N in _SMALL for c in _SMALL_CHECKS])
def test_kdyn_symmetries(N, check):
    """Translation by 1, 3 and G - 1 points along one axis; the cyclic relabelling of the axes (which maps the z, y and x pass kernels onto
    each other); exact scaling."""
    b = _kd_base(N)
    G = b["dom"].G
    if check == "scale":
        _kd_check_scaling(b)
    elif check == "perm":
        _kd_check_image(b, lambda v: kd_perm(v, G), "kdyn relabelling")
    else:
        axis = "xyz".index(check)
        for s in (1, 3, G - 1):
            sh = tuple(s if a == axis else 0 for a in range(3))
            _kd_check_image(b, lambda v: kd_roll(v, G, sh), "kdyn translation")
    if check == _SMALL_CHECKS[-1]:
        _drop_base()


_LARGE_CHECKS = ("roll", "perm", "scale")


@pytest.mark.parametrize("N,check", [(N, c) for N in _LARGE for c in _LARGE_CHECKS])
def test_kdyn_symmetries_large_sizes(N, check):
    """The tuned sizes the oracle is too slow for, the run-time-length 310 and the north-star 256, on full-spectrum data: one combined
    translation by (1, 3, G - 1), the relabelling, exact scaling."""
    b = _kd_base(N)
    G = b["dom"].G
    if check == "scale":
        _kd_check_scaling(b)
    elif check == "perm":
        _kd_check_image(b, lambda v: kd_perm(v, G), "kdyn large relabelling")
    else:
        _kd_check_image(b, lambda v: kd_roll(v, G, (1, 3, G - 1)), "kdyn large translation")
    if check == _LARGE_CHECKS[-1]:
        _drop_base()


@pytest.mark.parametrize("N", [16, 24, 22, 40, 192])      # 24: captured-graph replay; 22: odd G; 192: a large tuned size
@pytest.mark.parametrize("cost", ["Final", "Integrated"])
def test_kdyn_cost_is_a_quadratic_form_in_B0(N, cost):
    """Parallelogram law with a dirty direction; <gB, d> = (J(B+d) - J(B-d)) / 2 for the Discrete adjoint and SOLENOIDAL directions (the
    adjoint projects, so the identity does not hold for others).  Bounds: the J tolerance on every J involved, the gradient tolerance on
    |gB| |d|.  N = 192 keeps to the parallelogram: a solenoidal direction there costs 10 s of host FFTs."""
    _drop_base()
    dom = kdyn.KDynDomain(N)
    G = dom.G
    ctx = dom.context(RM, _kd_dt(G), NSTEPS, cost)
    B, U = _kd_inputs(G)
    d = (0.3 * np.random.RandomState(11).standard_normal(B.size) + 0.02) if G <= 96 else kd_cheap_field(G, 11, mean=0.02)
    Jp, Jm, Jd = ctx.forward([B + d, U]), ctx.forward([B - d, U]), ctx.forward([d, U])
    J = ctx.forward([B, U])
    scale = abs(Jp) + abs(Jm) + abs(J) + abs(Jd)
    defect = abs(0.5 * (Jp + Jm) - J - Jd)
    _note("kdyn parallelogram", defect / scale, 0.)
    assert defect <= JTOL * scale, (Jp, Jm, J, Jd)
    if N != 192:
        gB = ctx.adjoint(None, "Discrete")[0]
        gg = kdyn.Inner_Prod_3(gB, gB, dom)
        for d in (kdyn.synthetic_field(G, 5), 8. * kdyn.synthetic_field(G, 6)):
            Jp, Jm = ctx.forward([B + d, U]), ctx.forward([B - d, U])
            lhs = kdyn.Inner_Prod_3(gB, d, dom)
            bound = JTOL * 0.5 * (abs(Jp) + abs(Jm)) + GTOL * np.sqrt(gg * kdyn.Inner_Prod_3(d, d, dom))
            _note("kdyn <gB,d> (share of bound)", 0., abs(lhs - 0.5 * (Jp - Jm)) / bound)
            assert abs(lhs - 0.5 * (Jp - Jm)) <= bound, (lhs, 0.5 * (Jp - Jm))
    dom.drop_contexts()


def test_kdyn_symmetric_members_of_one_batch():
    """batch = 5 in one call: base, its translations along x, y and z, and its relabelling."""
    N, B_ = 16, 5
    dom = kdyn.KDynDomain(N)
    G = dom.G
    cost, adj = "Integrated", "Discrete"
    B, U = _kd_inputs(G)
    ops = [lambda v: v, lambda v: kd_roll(v, G, (1, 0, 0)), lambda v: kd_roll(v, G, (0, 3, 0)), lambda v: kd_roll(v, G, (0, 0, G - 1)),
           lambda v: kd_perm(v, G)]
    ctx = dom.context(RM, 1e-2, NSTEPS, cost, batch=B_)
    J = ctx.forward([np.concatenate([op(B) for op in ops]), np.concatenate([op(U) for op in ops])])
    gB, gU = (g.reshape(B_, -1) for g in ctx.adjoint(None, adj))
    for m in range(1, B_):
        dJ, dB, dU = abs(J[m] - J[0]) / abs(J[0]), rel(gB[m], ops[m](gB[0])), rel(gU[m], ops[m](gU[0]))
        _note("kdyn batch members", dJ, max(dB, dU))
        assert dJ <= JTOL and dB < GTOL and dU < GTOL, (m, dJ, dB, dU)
    dom.drop_contexts()


# ---- SH23 ----------------------------------------------------------------------------------------------------------------------------
# one length of every tuned family and its largest member; run-time lengths (1100: more than 64 KB of LDS)
_SH_TUNED = [16, 1024, 24, 384, 80, 640, 60, 960, 28, 896, 36, 576, 100, 800, 150, 600, 500]
_SH_ANY = [18, 21, 97, 333, 1100]


@pytest.mark.parametrize("Npts", _SH_TUNED + _SH_ANY)
def test_sh23_translation_and_reflection(Npts):
    """One batch of four per length — base, translation by 1 and by 7 points of the 2 Npts grid, reflection x -> -x — and both adjoint
    types (the oracle confirms the symmetries for both); the members of a batch are independent problems."""
    dom = sh23.SH23Domain(Npts)
    X = sh23.Generate_IC(0.0725, Npts=Npts, seed=42)[1] + 0.05 * np.random.RandomState(3).standard_normal(dom.G) + 0.01
    ops = [lambda v: v, lambda v: sh_roll(v, 1), lambda v: sh_roll(v, 7), sh_reflect]
    ctx = dom.context(0.1, 20, batch=4)
    J = ctx.forward([np.stack([op(X) for op in ops])])
    for adj in ("Discrete", "Continuous"):
        g = ctx.adjoint(None, adj)[0].reshape(4, -1)
        for m in range(1, 4):
            dJ, dg = abs(J[m] - J[0]) / abs(J[0]), rel(g[m], ops[m](g[0]))
            _note("sh23", dJ, dg)
            assert dJ <= JTOL and dg < GTOL, (adj, m, dJ, dg)
    ctx.close()


# ---- Poiseuille ----------------------------------------------------------------------------------------------------------------------
def _pz_check(dom, X, args, fwd, adj_solve, family):
    gs = dom.gshape
    J = fwd([X], *args); g = adj_solve([X], *args)[0]
    for sh in (1, 5):
        Xr = pz_roll(X, gs, sh)
        J1 = fwd([Xr], *args); g1 = adj_solve([Xr], *args)[0]
        dJ, dg = abs(J1 - J) / abs(J), rel(g1, pz_roll(g, gs, sh))
        _note(family, dJ, dg)
        assert dJ <= PTOL and dg < PTOL, (sh, dJ, dg)
    dom.drop_contexts()


@pytest.mark.parametrize("Nx,Nz,s", [(24, 24, 0), (30, 66, 1), (48, 36, 1), (60, 36, 0), (96, 48, 1)])
def test_poiseuille_discrete_translation_along_x(Nx, Nz, s):
    dom, U0 = pz.Generate_IC(Nx, Nz, E_0=0.02, seed=42)
    n = 5
    args = [dom, 500., 0.05, n, pz.GEN_BUFFER(Nx, Nz, dom, n), 5e-3, s, 1., 0.125]
    _pz_check(dom, U0[0], args, pz.FWD_Solve_Discrete, pz.ADJ_Solve_Discrete, "poiseuille discrete")


@pytest.mark.parametrize("Nx,Nz,s", [(16, 16, 0), (32, 24, 1)])
def test_poiseuille_continuous_translation_along_x(Nx, Nz, s):
    """The Continuous formulation on its 3/2 grid (the oracle confirms the symmetry there too)."""
    from oracle.poiseuille import PoiseuilleCntsOracle, synthetic_ic_cnts
    n = 5
    X = (10. if s == 1 else 1.) * synthetic_ic_cnts(PoiseuilleCntsOracle(Nx, Nz, dt=5e-3, N_ITERS=1, s=s, delta=0.3), 42)
    dom = pz.PoiseuilleDomain(Nx, Nz, continuous=True)
    args = [dom, 500., 0.05, n, pz.GEN_BUFFER(Nx, Nz, dom, n), 5e-3, s, 1., 0.3]
    _pz_check(dom, X, args, pz.FWD_Solve_Cnts, pz.ADJ_Solve_Cnts, "poiseuille continuous")
