"""The device paths at physical parameters OFF the reference scripts' values (tests/parameter_cases.py) against the oracle: Poiseuille at
Re = 200, Ri = 2, Prandtl = 0.5, Lx = 7, SH23 and SHB23 at other intervals and other a, and KDyn's refusal of a box that is not 2 pi.
test_parameters_oracle_cpu.py shows on the oracle alone that each of these parameters moves the gradient by >= 10 x RTOL in every case (and
by >= 1e-3 in at least one cost), so a kernel, an operator assembly or a context key that ignored one could not pass here.

Tolerances are the project's own: RTOL = 1e-6 on J, the gradient and <X, g> against the oracle; snapshots 1e-8 (Poiseuille, SHB23) and
1e-9 (SH23); 1e-11 for "same arithmetic, other summation order" in Poiseuille (the Pe identity); == where only exact quantities differ
(a translated interval, a repeated solve, a member of a batch).

Largest defects observed on an MI355X (a run with -s prints the table at its end):
    Poiseuille at P, Discrete (all paths, batch):     J 1.5e-15   gradient 1.4e-13   <X,g> 4.6e-15   snapshots 4.7e-15
    Poiseuille at P, Continuous:                      J 5.9e-16   gradient 2.7e-15   <X,g> 1.3e-15   snapshots 4.0e-15
    Poiseuille Pe identity across Re Pr = 1000:       J 7.5e-16   b snapshots 4.1e-16      (Re Pr = 500 differs by 1.0e-3 in J)
    SH23 cases:                                       J 5.5e-16   gradient 1.3e-15   <X,g> 6.6e-16   snapshots 1.4e-15
    SH23 closed form:                                 J 7.1e-16 of |J|, amplitude 5.1e-18 of eps
    SHB23 cases, Discrete:                            J 4.5e-15   gradient 1.3e-14   <X,g> 4.1e-15   snapshots 7.0e-15
    SHB23 cases, Continuous:                          J 1.7e-15   gradient 4.0e-15   <X,g> 1.3e-15   snapshots 4.3e-15
    SHB23 transforms 2.7e-16, weights 0
Translated intervals, the alternating context keys and the batch members were bit-exact.  With Prandtl = 1 handed to the device and 0.5 to
the oracle the 24 x 24, s = 1 case misses by 5.1e-3 in J and 8.5e-3 in the gradient.
"""
import numpy as np
import pytest

import parameter_cases as pc
from parameter_cases import rel
from spheremanopt_amd import _capi, kdyn, poiseuille as pz, shb23

pytestmark = pytest.mark.gpu
RTOL = 1e-6
PTOL = 1e-11

_WORST = {}


def _note(family, **defects):
    w = _WORST.setdefault(family, {})
    for k, v in defects.items():
        w[k] = max(w.get(k, 0.), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(_WORST):
        print("\nlargest defect  %-34s %s" % (fam, "   ".join("%s %.2e" % kv for kv in _WORST[fam].items())), end="")
    print()


# ---- Poiseuille at P against the oracle --------------------------------------------------------------------------------------------------
P = pc.POIS_P
X_DOMAIN = (0., P["Lx"])
_PZ_ORACLE = {}


def _pz_oracle(Nx, Nz, s, continuous, seed=42):
    """The oracle's J, gradient, snapshots 0, 1, -2, -1 and <X, g> at P: computed once per case, shared, read-only."""
    key = (Nx, Nz, s, continuous, seed)
    if key not in _PZ_ORACLE:
        o = pc.pois_oracle(Nx, Nz, s, continuous)
        X = pc.pois_input(Nx, Nz, continuous, seed)
        J = o.forward([X]); g = o.adjoint([X])[0]
        a = o.a if continuous else o.ax
        snaps = {(f, i): o.stack[f, :a, :, i].copy() for f in range(3) for i in (0, 1, -2, -1)}
        W = None if continuous else o.W
        g.setflags(write=False)
        _PZ_ORACLE[key] = dict(J=J, g=g, snaps=snaps, ip=o.inner(X, g), W=W)
    return _PZ_ORACLE[key]


def _pz_args(dom, buf, s, **params):
    p = dict(P, **params)
    return [dom, p["Re"], p["Ri"], pc.POIS_N, buf, pc.POIS_DT, s, p["Prandtl"], pc.POIS_DELTA]


def _pz_device(Nx, Nz, s, continuous, X, x_domain=X_DOMAIN, **params):
    """J, gradient, <X, g>, snapshots through the reference-signature callables on a fresh domain."""
    dom = pz.PoiseuilleDomain(Nx, Nz, X_domain=x_domain, continuous=continuous)
    buf = pz.GEN_BUFFER(Nx, Nz, dom, pc.POIS_N)
    args = _pz_args(dom, buf, s, **params)
    fwd, adj, ip = (pz.FWD_Solve_Cnts, pz.ADJ_Solve_Cnts, pz.Inner_Prod_Cnts) if continuous else \
                   (pz.FWD_Solve_Discrete, pz.ADJ_Solve_Discrete, pz.Inner_Prod_Discrete)
    J = fwd([X], *args)
    g = adj([X], *args)
    assert len(g) == 1 and g[0].shape == X.shape
    snaps = {(f, i): np.array(buf[k][:, :, i]) for f, k in enumerate(('u_fwd', 'w_fwd', 'b_fwd')) for i in (0, 1, -2, -1)}
    out = dict(J=J, g=g[0], snaps=snaps, ip=ip(X, g[0], dom), W=None if continuous else pz.weightMatrixDisc(dom))
    dom.drop_contexts()
    return out


def _pz_compare(got, ref, family):
    dJ, dg = abs(got["J"] - ref["J"]) / abs(ref["J"]), rel(got["g"], ref["g"])
    dip = abs(got["ip"] - ref["ip"]) / abs(ref["ip"])
    ds = max(rel(got["snaps"][k], ref["snaps"][k]) for k in ref["snaps"])
    print("%s: J %.2e  gradient %.2e  <X,g> %.2e  snapshots %.2e" % (family, dJ, dg, dip, ds))
    _note(family, J=dJ, gradient=dg, inner=dip, snapshots=ds)
    assert dJ <= RTOL, (got["J"], ref["J"])
    assert dg < RTOL, dg
    for k in ref["snaps"]:
        assert rel(got["snaps"][k], ref["snaps"][k]) < 1e-8, k
    assert dip <= RTOL, (got["ip"], ref["ip"])
    if ref["W"] is not None:
        assert np.array_equal(got["W"], ref["W"])


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("Nx,Nz", pc.POIS_DISCRETE_SIZES)
def test_poiseuille_discrete_at_P_vs_oracle(Nx, Nz, s):
    X = pc.pois_input(Nx, Nz)
    _pz_compare(_pz_device(Nx, Nz, s, False, X), _pz_oracle(Nx, Nz, s, False), "poiseuille P discrete")


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("Nx,Nz", pc.POIS_CNTS_SIZES)
def test_poiseuille_continuous_at_P_vs_oracle(Nx, Nz, s):
    X = pc.pois_input(Nx, Nz, True)
    _pz_compare(_pz_device(Nx, Nz, s, True, X), _pz_oracle(Nx, Nz, s, True), "poiseuille P continuous")


@pytest.mark.parametrize("name,value", [("SMO_POIS_XFFT", "0"), ("SMO_POIS_APPLY", "dense"), ("SMO_POIS_XPROD", "1")])
def test_poiseuille_alternative_paths_at_P_vs_oracle(name, value, monkeypatch):
    """The x phases as dense products, the dense operator stream and the products folded into the x transform: each against the ORACLE at P
    (the existing tests compare them with the default path at the default parameters only)."""
    monkeypatch.setenv(name, value)
    X = pc.pois_input(24, 24)
    _pz_compare(_pz_device(24, 24, 1, False, X), _pz_oracle(24, 24, 1, False), "poiseuille P discrete")


@pytest.mark.parametrize("s", [0, 1])
def test_poiseuille_batch_with_checkpoints_at_P(s):
    """batch = 3 with ckpt = 3 (n = 10: windows of two recomputed states, the last one shorter): every member against the oracle and, bit for
    bit, against a batch-1 keep-all solve."""
    Nx, Nz, n, B = 24, 24, pc.POIS_N, len(pc.POIS_BATCH_SEEDS)
    members = [pc.pois_input(Nx, Nz, seed=sd) for sd in pc.POIS_BATCH_SEEDS]
    refs = [_pz_oracle(Nx, Nz, s, False, sd) for sd in pc.POIS_BATCH_SEEDS]
    for i in range(B):
        for j in range(i):
            assert rel(refs[i]["g"], refs[j]["g"]) > 100 * RTOL, (i, j)
    dom = pz.PoiseuilleDomain(Nx, Nz, X_domain=X_DOMAIN, ckpt=3)
    ctx = dom.context(P["Re"], P["Ri"], n, pc.POIS_DT, s, P["Prandtl"], pc.POIS_DELTA, batch=B)
    assert ctx.get(0) == 3
    Xb = np.concatenate(members)
    J = ctx.forward([Xb])
    g = ctx.adjoint(None)[0].reshape(B, -1)
    ip = ctx.inner(Xb, g.reshape(-1))
    snaps = [[ctx.snapshot(i, b) for i in range(n + 1)] for b in range(B)]
    dom.drop_contexts()
    one = pz.PoiseuilleDomain(Nx, Nz, X_domain=X_DOMAIN)
    c1 = one.context(P["Re"], P["Ri"], n, pc.POIS_DT, s, P["Prandtl"], pc.POIS_DELTA)
    a = one.a
    for b in range(B):
        dJ, dg, dip = abs(J[b] - refs[b]["J"]) / abs(refs[b]["J"]), rel(g[b], refs[b]["g"]), abs(ip[b] - refs[b]["ip"]) / abs(refs[b]["ip"])
        _note("poiseuille P discrete", J=dJ, gradient=dg, inner=dip)
        assert dJ <= RTOL and dg < RTOL and dip <= RTOL, (b, dJ, dg, dip)
        for i in (0, 1, -2, -1):
            got = snaps[b][i].view(np.complex128).reshape(3, a, Nz)
            for f in range(3):
                assert rel(got[f], refs[b]["snaps"][(f, i)]) < 1e-8, (b, f, i)
        assert c1.forward([members[b]]) == J[b]
        assert np.array_equal(c1.adjoint(None)[0], g[b])
        assert c1.inner(members[b], g[b]) == ip[b]
        for i in range(n + 1):
            assert np.array_equal(c1.snapshot(i), snaps[b][i]), (b, i)
    one.drop_contexts()


@pytest.mark.parametrize("continuous,Nx,Nz", [(False, 24, 24), (True, 16, 16)])
def test_poiseuille_parameters_are_part_of_the_context_key(continuous, Nx, Nz):
    """One domain, P and P with Prandtl = 1 in turn: every result equals the first one of its parameter set bit for bit (no context of the
    other set is reused), and the two sets differ."""
    s = 1
    X = pc.pois_input(Nx, Nz, continuous)
    dom = pz.PoiseuilleDomain(Nx, Nz, X_domain=X_DOMAIN, continuous=continuous)
    buf = pz.GEN_BUFFER(Nx, Nz, dom, pc.POIS_N)
    fwd, adj = (pz.FWD_Solve_Cnts, pz.ADJ_Solve_Cnts) if continuous else (pz.FWD_Solve_Discrete, pz.ADJ_Solve_Discrete)
    first = {}
    for Pr in (P["Prandtl"], 1., P["Prandtl"], 1.):
        args = _pz_args(dom, buf, s, Prandtl=Pr)
        J = fwd([X], *args); g = adj([X], *args)[0]
        b = np.array(buf['b_fwd'][:, :, -1])
        if Pr not in first:
            first[Pr] = (J, g, b)
        else:
            assert J == first[Pr][0] and np.array_equal(g, first[Pr][1]) and np.array_equal(b, first[Pr][2]), Pr
    (J0, g0, b0), (J1, g1, b1) = first[P["Prandtl"]], first[1.]
    assert len(dom._ctx) == 2
    assert abs(J1 - J0) > 100 * RTOL * abs(J0) and rel(g1, g0) > 100 * RTOL and rel(b1, b0) > 100 * RTOL, (J0, J1, rel(g1, g0))
    dom.drop_contexts()


@pytest.mark.parametrize("continuous,Nx,Nz", [(False, 24, 24), (True, 16, 16)])
def test_poiseuille_pe_identity_on_the_device(continuous, Nx, Nz):
    """No oracle: X = 0, s = 1, so the cost is the mix-norm of a density that only diffuses, with 1 / (Re Pr).  (Re, Pr) = (500, 2), (1000, 1),
    (250, 4) must give the same J and b snapshots (1e-11); (500, 1) must not (1e-4).  A Re where Pe belongs fails the first, a Pr that is
    dropped the second."""
    dom = pz.PoiseuilleDomain(Nx, Nz, X_domain=X_DOMAIN, continuous=continuous)
    n = pc.POIS_N
    X = np.zeros(2 * dom.gshape[0] * dom.gshape[1])
    a = dom.a

    def solve(Re, Pr):
        ctx = dom.context(Re, P["Ri"], n, pc.POIS_DT, 1, Pr, pc.POIS_DELTA)
        J = ctx.forward([X])
        return J, np.stack([ctx.snapshot(i).view(np.complex128).reshape(3, a, Nz)[2] for i in range(n + 1)])

    J0, b0 = solve(*pc.POIS_PE_PAIRS[0])
    assert J0 != 0. and np.linalg.norm(b0[-1]) > 0.
    for Re, Pr in pc.POIS_PE_PAIRS[1:]:
        J, b = solve(Re, Pr)
        dJ, db = abs(J - J0) / abs(J0), max(rel(b[i], b0[i]) for i in range(n + 1))
        _note("poiseuille Pe identity", J=dJ, b=db)
        assert dJ <= PTOL and db <= PTOL, (Re, Pr, dJ, db)
    J, b = solve(*pc.POIS_PE_OTHER)
    print("Re Pr = 500 against 1000: J %.2e  b_n %.2e" % (abs(J - J0) / abs(J0), rel(b[-1], b0[-1])))
    assert abs(J - J0) > 1e-4 * abs(J0) and rel(b[-1], b0[-1]) > 1e-4
    dom.drop_contexts()


def test_poiseuille_translated_interval_is_the_same_problem():
    """Only x1 - x0 enters: (1.5, 8.5) equals (0, 7) bit for bit (both subtractions are exact)."""
    X = pc.pois_input(24, 24)
    a, b = _pz_device(24, 24, 1, False, X), _pz_device(24, 24, 1, False, X, x_domain=(1.5, 8.5))
    assert a["J"] == b["J"] and np.array_equal(a["g"], b["g"]) and a["ip"] == b["ip"] and np.array_equal(a["W"], b["W"])
    for k in a["snaps"]:
        assert np.array_equal(a["snaps"][k], b["snaps"][k]), k


# ---- SH23 --------------------------------------------------------------------------------------------------------------------------------
def _sh_ctx(Npts, interval, a, n=pc.SH23_N):
    return _capi.Context(_capi.SMO_SH23, Npts, interval, pc.SH23_DT, n, a)      # SH23Domain fixes a


@pytest.mark.parametrize("Npts", pc.SH23_NPTS)
@pytest.mark.parametrize("interval,a", pc.SH23_CASES)
def test_sh23_cases_vs_oracle(Npts, interval, a):
    from oracle.sh23 import SH23Oracle
    n = pc.SH23_N
    X = pc.sh23_input(Npts)
    o = SH23Oracle(Npts, interval=interval, dt=pc.SH23_DT, N_ITERS=n, a=a)
    Jo = o.forward([X])
    ctx = _sh_ctx(Npts, interval, a)
    J = ctx.forward([X])
    dJ = abs(J - Jo) / abs(Jo)
    assert dJ <= RTOL, (J, Jo)
    ds = max(rel(ctx.snapshot(i % (n + 1)).view(np.complex128), o.stack[:, i]) for i in (0, 1, n // 2, -1, -2))
    assert ds < 1e-9, ds
    for adj in ("Discrete", "Continuous"):
        g, go = ctx.adjoint(None, adj)[0], o.adjoint([X], adj)[0]
        ipo = o.inner(X, go)
        dg, dip = rel(g, go), abs(ctx.inner(X, g) - ipo) / abs(ipo)
        _note("sh23 cases", J=dJ, gradient=dg, inner=dip, snapshots=ds)
        assert g.shape == (2 * Npts,) and dg < RTOL and dip <= RTOL, (adj, dg, dip)
    ctx.close()


@pytest.mark.parametrize("Npts", pc.SH23_NPTS)
@pytest.mark.parametrize("interval,a", pc.SH23_CASES)
def test_sh23_known_answer_linear_growth_with_L_and_a(Npts, interval, a):
    """test_sh23_gpu.test_known_answer_linear_growth with L and a as arguments: r = (1/dt) / (1/dt + (1 - k_m^2)^2 - a), k_m = 2 pi m / L —
    not taken from the oracle.  Same tolerances."""
    eps, m, dt, n = 1e-9, 5, pc.SH23_DT, pc.SH23_N
    L = interval[1] - interval[0]
    G = 2 * Npts
    X = eps * np.cos(2. * np.pi * m * np.arange(G) / G)
    r = pc.sh23_growth(L, a, m, dt)
    ctx = _sh_ctx(Npts, interval, a)
    J = ctx.forward([X])
    expect = -dt * 0.5 * eps ** 2 * sum(r ** (2 * i) for i in range(n + 1))
    amp = abs(ctx.snapshot(n).view(np.complex128)[m])
    _note("sh23 closed form", J=abs(J - expect) / abs(expect), amplitude=abs(amp - 0.5 * eps * r ** n) / eps)
    assert abs(J - expect) < 1e-7 * abs(expect), (J, expect)
    assert abs(amp - 0.5 * eps * r ** n) < 1e-7 * eps
    ctx.close()


def test_sh23_translated_interval_is_the_same_problem():
    """(-3, 17.5) equals (0, 20.5) bit for bit: only x1 - x0 enters and both subtractions are exact."""
    a, n = pc.SH23_CASES[1][1], pc.SH23_N
    for Npts in pc.SH23_NPTS:
        X = pc.sh23_input(Npts)
        res = []
        for interval in ((-3., 17.5), (0., 20.5)):
            ctx = _sh_ctx(Npts, interval, a)
            res.append((ctx.forward([X]), ctx.adjoint(None, "Discrete")[0], ctx.adjoint(None, "Continuous")[0], ctx.snapshot(n)))
            ctx.close()
        assert res[0][0] == res[1][0] and all(np.array_equal(x, y) for x, y in zip(res[0][1:], res[1][1:]))


# ---- SHB23 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("continuous,N,n", [(False,) + sz for sz in pc.SHB23_DISCRETE_SIZES] + [(True,) + sz for sz in pc.SHB23_CNTS_SIZES])
@pytest.mark.parametrize("interval,a", pc.SHB23_CASES)
def test_shb23_cases_vs_oracle(continuous, N, n, interval, a):
    """SHBDomain fixes a, so through _capi.Context.  N = 512 (Discrete) and 256 modes (Continuous) run the multi-workgroup cluster."""
    X = pc.shb23_input(N, interval, a, continuous)
    o = pc.shb23_oracle(N, n, interval, a, continuous)
    Jo = o.forward([X]); go = o.adjoint([X])[0]
    ctx = _capi.Context(_capi.SMO_SHB23, N, interval, pc.SHB23_DT, n, a, cost=1 if continuous else 0)
    J = ctx.forward([X])
    g = ctx.adjoint(None, "Continuous" if continuous else "Discrete")[0]
    if N >= 256:
        assert ctx.get(2) > 1 and ctx.get(1) == 0                      # a cluster, and no fall-back to one workgroup
    ipo = o.inner(X, go)
    dJ, dg, dip = abs(J - Jo) / abs(Jo), rel(g, go), abs(ctx.inner(X, g) - ipo) / abs(ipo)
    ds = max(rel(ctx.snapshot(i % (n + 1)), o.stack[:, i]) for i in (0, 1, -1, -2))
    _note("shb23 cases %s" % ("continuous" if continuous else "discrete"), J=dJ, gradient=dg, inner=dip, snapshots=ds)
    assert dJ <= RTOL, (J, Jo)
    assert g.shape == X.shape and dg < RTOL, dg
    assert ds < 1e-8 and dip <= RTOL, (ds, dip)
    ctx.close()


@pytest.mark.parametrize("continuous,N", [(False, 64), (True, 32)])
@pytest.mark.parametrize("interval,a", pc.SHB23_CASES)
def test_shb23_transforms_and_weights_on_the_shifted_interval(continuous, N, interval, a):
    """The four smo_transform maps of a context on the shifted interval (Continuous: on its 2 N grid) and weightMatrixDisc against the
    oracle's helpers."""
    from oracle import shb23 as osh
    ctx = _capi.Context(_capi.SMO_SHB23, N, interval, pc.SHB23_DT, 2, a, cost=1 if continuous else 0)
    v = np.random.RandomState(5).standard_normal(ctx.vec_len)
    assert ctx.vec_len == (2 * N if continuous else N)
    for which, fun in enumerate((osh.transform, osh.transformInverse, osh.transformAdjoint, osh.transformInverseAdjoint)):
        d = rel(ctx.transform(which, v), fun(v))
        _note("shb23 helpers", transforms=d)
        assert d < 1e-13, (which, d)
    ctx.close()
    dom = shb23.SHBDomain(N, Z=interval, dealias=2 if continuous else 1)
    assert rel(dom.grid(0), osh.gauss_grid(N, interval)) < 1e-13
    d = rel(shb23.weightMatrixDisc(dom), osh.weights(osh.gauss_grid(N, interval)))
    _note("shb23 helpers", weights=d)
    assert d < 1e-13


# ---- KDyn: a box that is not 2 pi is refused -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [
    lambda X, N: _capi.Context(_capi.SMO_KDYN, N, X, 1e-3, 2, 1.0),
    lambda X, N: _capi.Context(_capi.SMO_KDYN, N, X, 1e-3, 2, 1.0, rank=0, world=2),
    lambda X, N: _capi.MultiContext(N, X, 1e-3, 2, 1.0, [0, 0]),
], ids=["one-gpu", "slab-rank", "multi-device"])
def test_kdyn_refuses_another_box_length(make):
    """The kernels carry the integer wavenumbers of a 2 pi box: (0, 4 pi) was silently solved as the 2 pi problem."""
    for N in (8, 16):
        with pytest.raises(_capi.SmoError, match="interval") as e:
            make(pc.KDYN_BAD_INTERVAL, N)
        assert e.value.code == 6 and _capi.ERR_NAMES[6] == "SMO_ERR_UNSUPPORTED"
    make(pc.KDYN_GOOD_INTERVALS[0], 16).close()                           # the same construction on (0, 2 pi) is accepted


def test_kdyn_translated_box_is_accepted():
    B, U = kdyn.synthetic_field(12, 1), kdyn.synthetic_field(12, 2)
    res = []
    for X in pc.KDYN_GOOD_INTERVALS:
        ctx = _capi.Context(_capi.SMO_KDYN, 8, X, 1e-3, 2, 1.0)
        res.append((ctx.forward([B, U]), ctx.snapshot(2)))
        ctx.close()
    assert res[0][0] == res[1][0] and res[0][0] != 0. and np.array_equal(res[0][1], res[1][1])
