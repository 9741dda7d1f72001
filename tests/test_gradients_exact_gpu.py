"""Oracle-free EXACT checks of the Discrete gradients of SH23 and Poiseuille and of the SH23 Hessian-vector product (tests/exact_grad_ops.py
states the identities, test_gradients_exact_cpu.py pins them on the CPU oracles and shows that they reject a 1e-8 error in one coefficient).

Needles.  <g, d> = sum_j w_j (J(X + j d) - J(X - j d)) with the stencil weights exact for the degree of J along the line: half-width 3^N for
    SH23 at every horizon N, 2 for Poiseuille (s = 0) at ONE step.  X is seeded white noise at the usual norm, d = 0.1 |X| d_unit, d_unit a
    single coefficient (SH23: k = 0, 1, Nc / 2, Nc - 1, two interior, a white direction; Poiseuille: u or w, (kx, kz) on the corners and edges
    of the de-aliased rectangle and inside it) or g / |g| (Poiseuille: cut to the band).  The base gradient comes from a batch-1 context, the
    2 m perturbed solves of every direction are members of one batched context.  Bound: JTOL = 1e-12 on every J the stencil reads plus
    GTOL = 1e-11 on |g| |d|; the bound itself must stay below SHARE = 1e-8 of |g| |d|.
Out of the band.  SH23: |<g, d>| within the bound and the stencil within JTOL of its scale (the gradient has no content there).
    Poiseuille: J unchanged within JTOL |J| (the gradient does have content there: the reference's, not asserted).
Hessian.  <W, HV> = sum_j w_j (<g(X + j V), W> - <g(X - j V), W>), m = 3^N, |V| = 0.1 |X|; bound GTOL on every gradient the stencil reads
    (times |W|) plus GTOL |HV| |W|, below SHARE |HV| |W|.

What is NOT here, because the identity is false there by the reference's design (characterised in test_gradients_exact_cpu.py): Poiseuille at
N_ITERS >= 2, SHB23, Poiseuille w needles at Ri != 0, and the mix-norm cost s = 1 — after one step it depends on w alone, through the analytic
derivative of the base profile where the adjoint has Dz rho_0: on the oracle the w needles miss by 2e-12 (30 x 66) .. 1e-2 (18 x 15) of
|g| |d| at every step of the ladder (0.1, 0.3, 1.0) |X|, and the bound is 1.6e-8, 5.4e-9, 1.6e-9 of |g| |d|: no step qualifies.

Largest figures observed on an MI355X (a run with -s prints the table at its end): the defect as a share of its bound, and the bound as a share
of |g| |d| (|HV| |W|), which must stay below 1e-8:
                                                  defect / bound    bound / (|g| |d|)
    SH23 n = 1, nine sizes:                           7.0e-5            1.7e-11
    SH23 n = 2, Npts 16, 54, 256, 1100:               6.8e-5            2.1e-11
    SH23 SMO_SH_ANY=1:                                4.1e-5            2.1e-11
    SH23 batch of 3, own a and horizon:               8.2e-5            2.1e-11
    SH23 Hessian (of |HV| |W|):                       2.1e-6            3.2e-10
    Poiseuille, six sizes, Ri = 0.05 and 0:           6.8e-5            1.5e-11
    Poiseuille 384 x 192:                             2.1e-4            1.5e-11
    Poiseuille dense apply / dense x / MB = 1, 4:     5.2e-5            1.5e-11
    Poiseuille SMO_POIS_XPROD=1:                      3.2e-5            1.5e-11
so the largest defect seen is 3e-15 of |g| |d| (Poiseuille 384 x 192).  Out of the band: SH23 |<g, d>| <= 2.3e-6 of its bound and the stencil
<= 1.3e-4 of JTOL times its scale; Poiseuille |J(X + t d) - J(X)| <= 4.4e-16 |J|.  40 tests, 4.3 s; the slowest is 384 x 192 (2.9 s).
"""
import numpy as np
import pytest

import band_ops as bo
import exact_grad_ops as eg
from exact_ops import JTOL, SHARE
from spheremanopt_amd import _capi, poiseuille as pz

pytestmark = pytest.mark.gpu
SEED = 42

_WORST = {}


def _note(family, share):
    _WORST[family] = max(_WORST.get(family, 0.), float(share))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(_WORST):
        print("\nlargest  %-52s %.2e" % (fam, _WORST[fam]), end="")
    print()


def _judge(family, failures, tag, g, d, m, Js, ip):
    """One in-band direction: within its bound, and the bound below SHARE of |g| |d|."""
    defect, bound, gd = eg.line_defect(g, d, m, Js, ip)
    _note("%s: defect / bound" % family, defect / bound)
    _note("%s: bound / (|g| |d|)" % family, bound / gd)
    if not (defect <= bound and bound < SHARE * gd):
        failures.append(tag + (defect / gd, bound / gd))


# ---- SH23 ----------------------------------------------------------------------------------------------------------------------------------
def _sh23_ctx(Npts, dt, horizons, avals):
    """One member per entry of horizons / avals."""
    ctx = _capi.Context(_capi.SMO_SH23, Npts, eg.SH23_BOX, dt, max(horizons), avals if len(avals) > 1 else avals[0])
    if len(set(horizons)) > 1:
        ctx.set_horizons(horizons)
    return ctx


def _sh23_members(family, Npts, horizons, avals=None):
    """Base: ONE context with a member per horizon (its own X, its own a); every member's gradient against its own stencil of half-width
    3^N_b, the perturbed solves of all members in one batched context with the member's a and horizon per solve."""
    B, G, dt = len(horizons), 2 * Npts, bo.sh23_dt(Npts)
    avals = list(avals or [eg.SH23_A] * B)
    Xs = [eg.white(G, sd, eg.SH23_NORM2, eg.sh23_inner) for sd in range(SEED, SEED + B)]
    base = _sh23_ctx(Npts, dt, horizons, avals)
    J0 = np.atleast_1d(base.forward([np.concatenate(Xs)]))
    gs = base.adjoint(None, "Discrete")[0].reshape(B, G)
    base.close()
    plan, points, hz, av = [], [], [], []
    for b in range(B):
        m = eg.degree_half_width("sh23", horizons[b])
        for name, inside, du in eg.sh23_directions(Npts) + [("aligned", True, eg.unit(gs[b], eg.sh23_inner))]:
            d = eg.scaled(du, Xs[b], eg.H, eg.sh23_inner)
            plan.append((b, name, inside, d, m))
            points += eg.line_points(Xs[b], d, m)
            hz += [horizons[b]] * (2 * m)
            av += [avals[b]] * (2 * m)
    ctx = _sh23_ctx(Npts, dt, hz, av)
    Js = list(np.atleast_1d(ctx.forward([np.concatenate(points)])))
    ctx.close()
    failures = []
    for b, name, inside, d, m in plan:
        mine, Js = Js[:2 * m], Js[2 * m:]
        if inside:
            _judge(family, failures, (b, name), gs[b], d, m, mine, eg.sh23_inner)
        else:
            gd_, st, bound, jscale = eg.blind_defect(gs[b], d, m, mine, eg.sh23_inner)
            _note("%s, out of the band: |<g, d>| / bound" % family, gd_ / bound)
            _note("%s, out of the band: stencil / (JTOL scale)" % family, st / jscale)
            if not (gd_ <= bound and st <= jscale and max(abs(J - J0[b]) for J in mine) <= JTOL * abs(J0[b])):
                failures.append((b, name, "blind", gd_ / bound, st / jscale))
    assert not failures, failures


@pytest.mark.parametrize("Npts", bo.SH23_SIZES)
def test_sh23_needles_one_step(Npts):
    _sh23_members("SH23 n = 1", Npts, [1])


@pytest.mark.parametrize("Npts", [16, 54, 256, 1100])
def test_sh23_needles_two_steps(Npts):
    """Half-width 9: 18 solves per direction."""
    _sh23_members("SH23 n = 2", Npts, [2])


def test_sh23_needles_run_time_length_kernels_at_a_tuned_size(monkeypatch):
    monkeypatch.setenv("SMO_SH_ANY", "1")
    for n in (1, 2):
        _sh23_members("SH23 SMO_SH_ANY=1", bo.SH23_ANY_SIZE, [n])


@pytest.mark.parametrize("Npts", [64, 54])
def test_sh23_needles_members_with_their_own_input_parameter_and_horizon(Npts):
    _sh23_members("SH23 batch of 3, own a and horizon", Npts, [2, 1, 2], avals=[-0.3, -0.2, -0.4])


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("Npts", [64, 1024, 54])
def test_sh23_hessian_is_the_exact_derivative_of_the_gradient(Npts, n):
    """64: four transforms side by side in the second-order adjoint sweep; 1024: two rounds of two; 54: the any-length kernels."""
    G, dt, ip = 2 * Npts, bo.sh23_dt(Npts), eg.sh23_inner
    m = eg.degree_half_width("sh23", n)
    X = eg.white(G, SEED, eg.SH23_NORM2, ip)
    rs = np.random.RandomState(11)
    V, W = eg.scaled(eg.unit(rs.standard_normal(G), ip), X, eg.SH23_HESSIAN_H, ip), eg.unit(rs.standard_normal(G), ip)
    base = _sh23_ctx(Npts, dt, [n], [eg.SH23_A])
    base.forward([X])
    (HV,), _ = base.hessvec([V])
    base.close()
    ctx = _sh23_ctx(Npts, dt, [n] * (2 * m), [eg.SH23_A] * (2 * m))
    ctx.forward([np.concatenate(eg.line_points(X, V, m))])
    grads = ctx.adjoint(None, "Discrete")[0].reshape(2 * m, G)
    ctx.close()
    defect, bound, hw = eg.hessian_line_defect(W, HV, grads[0::2], grads[1::2], m, ip)
    _note("SH23 Hessian: defect / bound", defect / bound)
    _note("SH23 Hessian: bound / (|HV| |W|)", bound / hw)
    assert defect <= bound and bound < SHARE * hw, (defect / hw, bound / hw)


# ---- Poiseuille, s = 0, one step ---------------------------------------------------------------------------------------------------------------
def _pois_case(family, Nx, Nz, Ri, comps, which="all", how="batch"):
    """how = "batch": every perturbed solve a member of one batched context; "single": one call each on the base context."""
    ip = eg.pois_inner_product(Nx, Nz)
    X = eg.white(2 * Nx * Nz, SEED, eg.POIS_NORM2, ip)
    dom = pz.PoiseuilleDomain(Nx, Nz)
    args = (bo.POIS_RE, Ri, 1, 5e-3, 0, bo.POIS_PR, bo.POIS_DELTA)
    base = dom.context(*args)
    J0 = base.forward([X])
    g = base.adjoint(None)[0]
    m = eg.degree_half_width("pois", 1)
    dirs = eg.pois_directions(Nx, Nz, comps, which) + [("aligned", True, eg.unit(eg.pois_band_project(g, Nx, Nz, comps), ip))]
    plan = [(name, inside, eg.scaled(du, X, eg.H, ip)) for name, inside, du in dirs]
    points = [Y for _, _, d in plan for Y in eg.line_points(X, d, m)]
    if how == "batch":
        Js = list(dom.context(*args, batch=len(points)).forward([np.concatenate(points)]))
    else:
        Js = [base.forward([Y]) for Y in points]
    dom.drop_contexts()
    failures = []
    for i, (name, inside, d) in enumerate(plan):
        mine = Js[2 * m * i:2 * m * (i + 1)]
        if inside:
            _judge(family, failures, (name,), g, d, m, mine, ip)
        else:
            blind = max(abs(J - J0) for J in mine) / abs(J0)
            _note("%s, out of the band: |J(X + t d) - J(X)| / |J|" % family, blind)
            if blind > JTOL:
                failures.append((name, "blind", blind))
    assert not failures, failures


POIS_SIZES = [(24, 24), (30, 66), (18, 15), (42, 27), (96, 48), (90, 21)]     # ragged z tile, odd Nz, no x-FFT instantiation (42, 90)
POIS_VARIANT = (30, 66)


@pytest.mark.parametrize("Ri,comps", [(bo.POIS_RI, "u"), (0., "uw")], ids=["Ri0.05-u", "Ri0-uw"])
@pytest.mark.parametrize("Nx,Nz", POIS_SIZES)
def test_poiseuille_needles_one_step(Nx, Nz, Ri, comps):
    _pois_case("Poiseuille", Nx, Nz, Ri, comps)


def test_poiseuille_needles_one_step_at_the_bench_grid():
    """384 x 192: the four corners of the band in u and in w, and the aligned direction."""
    _pois_case("Poiseuille 384 x 192", 384, 192, 0., "uw", which="corners")


@pytest.mark.parametrize("name,value", [("SMO_POIS_APPLY", "dense"), ("SMO_POIS_XFFT", "0"), ("SMO_POIS_APPLY_MB", "1"), ("SMO_POIS_APPLY_MB", "4")])
def test_poiseuille_needles_alternative_paths(name, value, monkeypatch):
    monkeypatch.setenv(name, value)
    _pois_case("Poiseuille %s=%s" % (name, value), *POIS_VARIANT, 0., "uw")
    _pois_case("Poiseuille %s=%s" % (name, value), *POIS_VARIANT, bo.POIS_RI, "u", which="corners")


def test_poiseuille_needles_products_folded_into_the_x_transform(monkeypatch):
    """SMO_POIS_XPROD=1 is built for batch 1: the solves one by one, corner needles."""
    monkeypatch.setenv("SMO_POIS_XPROD", "1")
    _pois_case("Poiseuille SMO_POIS_XPROD=1", *POIS_VARIANT, 0., "uw", which="corners", how="single")
