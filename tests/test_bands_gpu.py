"""SH23, SHB23 and Poiseuille on the device against the oracle, band by band, with full-spectrum (white) inputs: band_ops.py has the inputs,
the criterion and the case tables, test_bands_oracle_cpu.py shows on the oracle that every band of these cases carries weight and that the
criterion sees a 1e-5 defect in any single band.  The cases sit where the kernels have their edges: the truncation index after
de-aliasing and the last retained mode, the last twiddles of the mixed-radix and run-time-length LDS FFTs (SH23 21, 54, 96, 100, 112, 1100),
the last rows of the tau operators, the SHB23 cluster with its remainder workgroup (1023) and with the cluster off, one workgroup per member
at a cluster size (batch of 3 at N = 512), the ragged last z tile of the Chebyshev GEMMs (30 x 66) on every alternative Poiseuille path.

Per case: J and <X, g> at RTOL = 1e-6; band_defects of snapshots 0, 1, n - 1, n of every state field at 1e-9 (SH23) / 1e-8 (SHB23,
Poiseuille); band_defects of the spectral view of every gradient component at RTOL (and the whole gradient, as everywhere else); the
de-aliased rows of the Poiseuille Discrete snapshots == 0.  FLOOR = 1e-3.  The oracle's answers are computed once per case and are read-only.

Largest defects observed on an MI355X (a run with -s prints the table at its end):
    SH23 (every size, both adjoints):        J 2.4e-16   <X,g> 4.8e-16   snapshot bands 6.9e-16   gradient bands 1.2e-15
    SH23 batch, horizons:                    J 2.1e-16   <X,g> 3.6e-16   snapshot bands 6.4e-16   gradient bands 9.2e-16
    SHB23 Discrete (cluster, one workgroup): J 4.7e-16   <X,g> 4.6e-16   snapshot bands 5.9e-13   their spectra 1.3e-10   gradient bands 4.3e-14
    SHB23 Continuous:                        J 6.2e-16   <X,g> 6.0e-16   snapshot bands 6.0e-15   gradient bands 6.0e-15
    SHB23 batch:                             J 5.7e-16   <X,g> 4.3e-16   snapshot bands 1.9e-13   their spectra 2.2e-11   gradient bands 8.4e-15
    Poiseuille Discrete (all paths, batch):  J 2.1e-15   <X,g> 4.7e-13   snapshot bands 2.2e-12   gradient bands 5.9e-10
    Poiseuille Continuous:                   J 5.4e-16   <X,g> 1.3e-14   snapshot bands 3.3e-14   gradient bands 1.7e-12
The 1.3e-10 belongs to bands of the spectrum of SHB23 Discrete snapshot 1 that hold less than FLOOR (N >= 512): 1.3e-13 of the snapshot.
The 5.9e-10 is the band (x 0, z 1) of g_w at 30 x 66, s = 1, the same figure on the HODLR, dense, x-FFT, dense-x and folded-product paths
and in the batch, so it is a property of the comparison (the oracle solves dense 462 x 462 tau systems, the device its own LU), not of a path.
With the defects of test_bands_oracle_cpu.py planted by hand into device results (the gradient's top band times 1 + 1e-4 at SH23 1024,
SHB23 512 and Poiseuille 96 x 48, the top band of an SH23 snapshot zeroed) the band assertion of that quantity fails with 1.0e-4 and 1.0.
"""
import numpy as np
import pytest

import band_ops as bo
from band_ops import RTOL, band_defects, rel
from spheremanopt_amd import poiseuille as pz, sh23, shb23

pytestmark = pytest.mark.gpu
N = bo.N_STEPS

_WORST = {}


def _note(family, **defects):
    w = _WORST.setdefault(family, {})
    for k, v in defects.items():
        w[k] = max(w.get(k, 0.), float(v))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(_WORST):
        print("\nlargest defect  %-28s %s" % (fam, "   ".join("%s %.2e" % kv for kv in _WORST[fam].items())), end="")
    print()


def _scalars(family, J, Jo, ip, ipo):
    dJ, dip = abs(J - Jo) / abs(Jo), abs(ip - ipo) / abs(ipo)
    print("%s: J %.2e  <X,g> %.2e" % (family, dJ, dip))
    _note(family, J=dJ, inner=dip)
    assert dJ <= RTOL, (J, Jo)
    assert dip <= RTOL, (ip, ipo)


def _bands(family, what, got, ref, bands, tol, key):
    d = band_defects(got, ref, bands)
    print("%s: %s %s  bands %s" % (family, key, what, " ".join("%.1e" % x for x in d)))
    _note(family, **{key: max(d)})
    assert max(d) < tol, (what, d)


def _snapshot_indices(n):
    return sorted({0, 1, n - 1, n})


# ---- SH23 --------------------------------------------------------------------------------------------------------------------------------
def _sh23_check(family, r, n, J, snapshot, grads, inner):
    """snapshot(i) -> Nc complex coefficients; grads {adjoint type: g}; inner(g) -> <X, g>."""
    for i in _snapshot_indices(n):
        _bands(family, "snapshot %d" % i, snapshot(i), r["snaps"][:, i], r["bands"], bo.SNAP_TOL["sh23"], "snapshots")
    for adj, g in grads.items():
        ref = r[adj]
        _scalars(family, J, r["J"], inner(g), ref["ip"])
        assert g.shape == ref["g"].shape
        _bands(family, "gradient " + adj, bo.sh23_grad_view(r["o"], g), ref["view"], r["bands"], RTOL, "gradient")
        assert rel(g, ref["g"]) < RTOL


def _sh23_callables(Npts, adj):
    r = bo.sh23_ref(Npts)
    dom = sh23.SH23Domain(Npts)
    buf = sh23.GEN_BUFFER(dom, N)
    args = [dom, r["dt"], N, N, buf, None, adj]
    J = sh23.FWD_Solve_IVP_Lin([r["X"]], *args)
    g = sh23.ADJ_Solve_IVP_Lin([r["X"]], *args)
    assert len(g) == 1
    _sh23_check("sh23", r, N, J, lambda i: buf['A_fwd'][:, i], {adj: g[0]}, lambda v: sh23.Inner_Prod(r["X"], v, dom))
    dom.drop_contexts()


@pytest.mark.parametrize("adj", bo.SH23_ADJOINTS)
@pytest.mark.parametrize("Npts", bo.SH23_SIZES)
def test_sh23_bands(Npts, adj):
    _sh23_callables(Npts, adj)


@pytest.mark.parametrize("adj", bo.SH23_ADJOINTS)
def test_sh23_bands_run_time_length_kernels_at_a_tuned_size(adj, monkeypatch):
    monkeypatch.setenv("SMO_SH_ANY", "1")
    _sh23_callables(bo.SH23_ANY_SIZE, adj)


def _sh23_members(Npts, horizons):
    """A batch of the BATCH_SEEDS inputs, member b with horizons[b] steps."""
    refs = [bo.sh23_ref(Npts, nb, sd) for nb, sd in zip(horizons, bo.BATCH_SEEDS)]
    B, G = len(refs), refs[0]["X"].size
    dom = sh23.SH23Domain(Npts)
    ctx = dom.context(refs[0]["dt"], horizons if len(set(horizons)) > 1 else horizons[0], batch=B)
    X = np.concatenate([r["X"] for r in refs])
    J = ctx.forward([X])
    g = {adj: ctx.adjoint(None, adj)[0].reshape(B, G) for adj in bo.SH23_ADJOINTS}
    ip = {adj: ctx.inner(X, g[adj].reshape(-1)) for adj in bo.SH23_ADJOINTS}
    for b, r in enumerate(refs):
        for adj in bo.SH23_ADJOINTS:
            _sh23_check("sh23 batch", r, horizons[b], J[b], lambda i: ctx.snapshot(i, b).view(np.complex128), {adj: g[adj][b]},
                        lambda v: ip[adj][b])
    dom.drop_contexts()


@pytest.mark.parametrize("Npts", bo.SH23_BATCH_SIZES)
def test_sh23_bands_batch(Npts):
    _sh23_members(Npts, (N,) * len(bo.BATCH_SEEDS))


def test_sh23_bands_members_with_their_own_horizons():
    _sh23_members(*bo.SH23_HORIZONS)


# ---- SHB23 -------------------------------------------------------------------------------------------------------------------------------
def _shb23_check(family, r, continuous, J, snapshot, g, ip):
    tol = bo.SNAP_TOL["shb23"]
    for i in _snapshot_indices(N):
        got, ref = snapshot(i), r["snaps"][:, i]
        _bands(family, "snapshot %d" % i, got, ref, r["bands"], tol, "snapshots")
        if not continuous:                                   # grid states: their spectrum as well (damped by the step: the floor rule)
            _bands(family, "spectrum of snapshot %d" % i, bo.shb23_snap_view(got, False), bo.shb23_snap_view(ref, False), r["bands"], tol, "spectra")
    _scalars(family, J, r["J"], ip, r["ip"])
    assert g.shape == r["g"].shape
    _bands(family, "gradient", bo.shb23_grad_view(r["o"], g, continuous), r["view"], r["bands"], RTOL, "gradient")
    assert rel(g, r["g"]) < RTOL


def _shb23_callables(Npts, continuous, workgroups):
    """workgroups: 'cluster' (more than one, and no fall-back), 'one', or None (whatever the size takes)."""
    r = bo.shb23_ref(Npts, continuous)
    dom = shb23.SHBDomain(Npts, dealias=2 if continuous else 1)
    buf = shb23.GEN_BUFFER(Npts, dom, N)
    fwd, adj, inner = (shb23.FWD_Solve_IVP_Cnts, shb23.ADJ_Solve_IVP_Cnts, shb23.Inner_Prod_Cnts) if continuous else \
                      (shb23.FWD_Solve_IVP_Discrete, shb23.ADJ_Solve_IVP_Discrete, shb23.Inner_Prod_Discrete)
    J = fwd([r["X"]], dom, buf, N, r["dt"])
    g = adj([r["X"]], dom, buf, N, r["dt"])
    assert len(g) == 1
    ctx = dom.context(r["dt"], N)
    if workgroups == "cluster":
        assert ctx.get(2) > 1 and ctx.get(1) == 0
    elif workgroups == "one":
        assert ctx.get(2) == 1
    family = "shb23 %s" % ("continuous" if continuous else "discrete")
    _shb23_check(family, r, continuous, J, lambda i: buf['A_fwd'][:, i], g[0], inner(r["X"], g[0], dom))
    dom.drop_contexts()


@pytest.mark.parametrize("Npts", bo.SHB23_SIZES)
def test_shb23_discrete_bands(Npts):
    _shb23_callables(Npts, False, "cluster" if Npts >= 256 else "one")


@pytest.mark.parametrize("Npts", bo.SHB23_NO_CLUSTER)
def test_shb23_discrete_bands_one_workgroup_at_a_cluster_size(Npts, monkeypatch):
    monkeypatch.setenv("SMO_SHB_CLUSTER", "0")
    _shb23_callables(Npts, False, "one")


def test_shb23_discrete_bands_run_time_length_kernels_at_a_tuned_size(monkeypatch):
    monkeypatch.setenv("SMO_SHB_ANY", "1")
    _shb23_callables(bo.SHB23_ANY_SIZE, False, None)


@pytest.mark.parametrize("Npts", bo.SHB23C_SIZES)
def test_shb23_continuous_bands(Npts):
    _shb23_callables(Npts, True, "cluster" if Npts >= 256 else "one")


@pytest.mark.parametrize("continuous,Npts", [(False, n) for n in bo.SHB23_BATCH_SIZES] + [(True, n) for n in bo.SHB23C_BATCH_SIZES])
def test_shb23_bands_batch(continuous, Npts):
    """One workgroup per member, also where a single problem of that size takes the cluster (N = 512, 256 modes)."""
    refs = [bo.shb23_ref(Npts, continuous, N, sd) for sd in bo.BATCH_SEEDS]
    B = len(refs)
    dom = shb23.SHBDomain(Npts, dealias=2 if continuous else 1)
    ctx = dom.context(refs[0]["dt"], N, batch=B)
    X = np.concatenate([r["X"] for r in refs])
    J = ctx.forward([X])
    g = ctx.adjoint(None, "Continuous" if continuous else "Discrete")[0]
    ip = ctx.inner(X, g)
    assert ctx.get(2) == 1
    g = g.reshape(B, -1)
    for b, r in enumerate(refs):
        _shb23_check("shb23 batch", r, continuous, J[b], lambda i: ctx.snapshot(i, b), g[b], ip[b])
    dom.drop_contexts()


# ---- Poiseuille --------------------------------------------------------------------------------------------------------------------------
def _pz_check(family, r, n, continuous, J, snapshot, g, ip):
    """snapshot(f, i) -> (rows, Nz) complex coefficients of field f (u, w, b)."""
    o, keep = r["o"], r["xkeep"]
    for i in _snapshot_indices(n):
        for f, name in enumerate("uwb"):
            got, ref = snapshot(f, i), r["snaps"][(f, i)]
            assert got.shape == ref.shape
            _bands(family, "%s snapshot %d" % (name, i), got[:keep], ref[:keep], r["bands_snap"], bo.SNAP_TOL["pois"], "snapshots")
            assert not np.any(got[keep:]), (name, i)               # the de-aliased rows (Discrete): exactly zero, as on the oracle
    _scalars(family, J, r["J"], ip, r["ip"])
    assert g.shape == r["g"].shape
    for name, got, ref in zip("uw", bo.pois_grad_views(o, g, continuous), r["views"]):
        _bands(family, "gradient " + name, got, ref, r["bands_grad"], RTOL, "gradient")
    assert rel(g, r["g"]) < RTOL


def _pz_callables(Nx, Nz, n, s, continuous, ckpt=1):
    r = bo.pois_ref(Nx, Nz, n, s, continuous)
    dom = pz.PoiseuilleDomain(Nx, Nz, continuous=continuous, ckpt=ckpt)
    buf = pz.GEN_BUFFER(Nx, Nz, dom, n)
    args = [dom, bo.POIS_RE, bo.POIS_RI, n, buf, r["dt"], s, bo.POIS_PR, bo.POIS_DELTA]
    fwd, adj, inner = (pz.FWD_Solve_Cnts, pz.ADJ_Solve_Cnts, pz.Inner_Prod_Cnts) if continuous else \
                      (pz.FWD_Solve_Discrete, pz.ADJ_Solve_Discrete, pz.Inner_Prod_Discrete)
    J = fwd([r["X"]], *args)
    g = adj([r["X"]], *args)
    assert len(g) == 1
    if ckpt != 1:
        assert dom.context(*args[1:4], r["dt"], s, bo.POIS_PR, bo.POIS_DELTA).get(0) == ckpt
    keys = ('u_fwd', 'w_fwd', 'b_fwd')
    _pz_check("poiseuille %s" % ("continuous" if continuous else "discrete"), r, n, continuous, J, lambda f, i: buf[keys[f]][:, :, i], g[0],
              inner(r["X"], g[0], dom))
    dom.drop_contexts()


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("Nx,Nz,n", bo.POIS_SIZES)
def test_poiseuille_discrete_bands(Nx, Nz, n, s):
    _pz_callables(Nx, Nz, n, s, False)


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("name,value", bo.POIS_VARIANTS)
def test_poiseuille_discrete_bands_alternative_paths(name, value, s, monkeypatch):
    monkeypatch.setenv(name, value)
    _pz_callables(*bo.POIS_VARIANT_SIZE, s, False)


@pytest.mark.parametrize("s", [0, 1])
def test_poiseuille_discrete_bands_with_checkpoints(s):
    _pz_callables(*bo.POIS_VARIANT_SIZE, s, False, ckpt=2)


@pytest.mark.parametrize("s", [0, 1])
def test_poiseuille_discrete_bands_batch(s):
    Nx, Nz, n = bo.POIS_VARIANT_SIZE
    refs = [bo.pois_ref(Nx, Nz, n, s, False, sd) for sd in bo.BATCH_SEEDS]
    B = len(refs)
    dom = pz.PoiseuilleDomain(Nx, Nz)
    ctx = dom.context(bo.POIS_RE, bo.POIS_RI, n, refs[0]["dt"], s, bo.POIS_PR, bo.POIS_DELTA, batch=B)
    X = np.concatenate([r["X"] for r in refs])
    J = ctx.forward([X])
    g = ctx.adjoint(None)[0]
    ip = ctx.inner(X, g)
    g = g.reshape(B, -1)
    for b, r in enumerate(refs):
        _pz_check("poiseuille batch", r, n, False, J[b], lambda f, i: ctx.snapshot(i, b).view(np.complex128).reshape(3, dom.a, Nz)[f], g[b], ip[b])
    dom.drop_contexts()


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("Nx,Nz,n", bo.POISC_SIZES)
def test_poiseuille_continuous_bands(Nx, Nz, n, s):
    _pz_callables(Nx, Nz, n, s, True)
