"""SH23 Hessian-vector products on the device (smo_hessvec*: sh23_tangent_kernel / sh23_soa_kernel and their any-length forms).

(1) against the NumPy restatement of hessvec_ops.py (pinned on the CPU by test_hessvec_oracle_cpu.py) on every code path: instantiated
lengths with four transforms side by side, instantiated lengths above the LDS threshold (two rounds of two), any-length kernels incl. the
LDS opt-in, SMO_SH_ANY=1 against the instantiated kernels; (2) oracle-free identities on the device alone; (3) batch, per-member a and
per-member horizons against batch-1 contexts, bit for bit, host and device vectors; (4) state and refusals; (5) independence of what device
memory held (SMO_POISON); (6) the second-order example.

Observed on an MI355X (30 tests, 1.3 s): rel(H.V) against the restatement 2.6e-16 .. 1.3e-15 and |dJ - ref| / |ref| <= 1.3e-14 over the ten
cases; any-length against instantiated kernels 4e-16; |dJ - <V, grad>| <= 1e-17 and |<W,HV> - <V,HW>| <= 8e-18 against bounds of 1e-11;
central-difference error ratios 99.97 and 100.00; third-remainder slopes 3.028, 3.014, 3.007 (Npts 64) and 3.020, 3.010, 3.005 (Npts 54); the
example: 17 Lanczos steps, theta_min = -0.7569552527 on the device and on the restatement, residuals 3e-15.
"""
import functools
import gc

import numpy as np
import pytest

import hessvec_ops as ho
from oracle.sh23 import synthetic_ic
from spheremanopt_amd import _capi, hessian, sh23
from spheremanopt_amd.devvec import DeviceVector

pytestmark = pytest.mark.gpu

RTOL = 1e-6
BOX = (0., 12. * np.pi)
TUNED_WIDE = [(16, 0.1, 3), (32, 0.05, 17), (64, 0.1, 40), (96, 0.1, 20), (600, 0.02, 4), (768, 0.02, 4)]
TUNED_ROUNDS = [(800, 0.02, 6), (1024, 0.02, 6)]
ANY = [(21, 0.1, 12), (54, 0.1, 20), (97, 0.1, 10), (1100, 0.02, 4)]


def _ctx(Npts, dt, N, a=sh23.A_PARAM, batch=1):
    return _capi.Context(_capi.SMO_SH23, Npts, BOX, dt, N, a, batch=batch)


@functools.lru_cache(maxsize=None)
def _ref(Npts, dt, N, a=sh23.A_PARAM, seeds=(ho.SEED_X, ho.SEED_V)):
    """(f, df, grad, HV) of the restatement; computed once per case and shared (the arrays are read only)."""
    o = ho.oracle(Npts, dt, N, a)
    X, V = (synthetic_ic(2 * Npts, s, ho.E0) for s in seeds)
    df, g, HV = ho.hessvec(o, X, V)
    f = o.forward([X])
    for arr in (g, HV):
        arr.setflags(write=False)
    return f, df, g, HV


# ---- (1) against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Npts,dt,N", TUNED_WIDE + TUNED_ROUNDS + ANY)
def test_against_the_restatement(Npts, dt, N):
    X, V, _ = ho.inputs(Npts)
    f_ref, df_ref, g_ref, HV_ref = _ref(Npts, dt, N)
    ctx = _ctx(Npts, dt, N)
    f = ctx.forward([X])
    (HV,), dJ = ctx.hessvec([V])
    g = ctx.adjoint()[0]
    ctx.close()
    print("Npts %d: rel(HV) %.2e  |dJ - ref|/|ref| %.2e  rel(grad) %.2e" % (Npts, ho.rel(HV, HV_ref), abs(dJ - df_ref) / abs(df_ref), ho.rel(g, g_ref)))
    assert HV.shape == (2 * Npts,) and isinstance(dJ, float)
    assert ho.rel(HV, HV_ref) < RTOL
    assert abs(dJ - df_ref) <= RTOL * abs(df_ref)
    assert abs(f - f_ref) <= RTOL * abs(f_ref) and ho.rel(g, g_ref) < RTOL


@pytest.mark.parametrize("Npts,dt,N", [(64, 0.1, 40), (96, 0.1, 20)])
def test_any_length_kernels_match_the_instantiated_ones(Npts, dt, N, monkeypatch):
    X, V, _ = ho.inputs(Npts)
    res = []
    for force in ("0", "1"):
        monkeypatch.setenv("SMO_SH_ANY", force)
        ctx = _ctx(Npts, dt, N)
        ctx.forward([X])
        (HV,), dJ = ctx.hessvec([V])
        res.append((HV, dJ))
        ctx.close()
    (H0, d0), (H1, d1) = res
    print("Npts %d: any vs tuned rel(HV) %.2e  dJ %.2e" % (Npts, ho.rel(H1, H0), abs(d1 - d0) / abs(d0)))
    assert ho.rel(H1, H0) < 1e-11 and abs(d1 - d0) <= 1e-11 * abs(d0)
    assert ho.rel(H1, _ref(Npts, dt, N)[3]) < RTOL


# ---- (2) oracle-free, on the device alone ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(64, 0.1, 40), (54, 0.1, 20)], ids=["64-tuned", "54-any"])
def dev(request):
    Npts, dt, N = request.param
    X, V, W = ho.inputs(Npts)
    ctx = _ctx(Npts, dt, N)
    ctx.forward([X])
    g = ctx.adjoint()[0]
    (HV,), dJ = ctx.hessvec([V])
    (HW,), _ = ctx.hessvec([W])
    yield {"ctx": ctx, "X": X, "V": V, "W": W, "g": g, "HV": HV, "HW": HW, "dJ": dJ}
    ctx.close()


def _norm(ctx, x):
    return ctx.inner(x, x) ** 0.5


def test_directional_derivative_is_the_gradients(dev):
    ctx = dev["ctx"]
    d = ctx.inner(dev["V"], dev["g"])
    bound = 1e-10 * _norm(ctx, dev["V"]) * _norm(ctx, dev["g"])
    print("dJ %.16e  <V, grad> %.16e  diff %.2e  bound %.2e" % (dev["dJ"], d, abs(dev["dJ"] - d), bound))
    assert abs(dev["dJ"] - d) <= bound


def test_symmetry(dev):
    ctx = dev["ctx"]
    a, b = ctx.inner(dev["W"], dev["HV"]), ctx.inner(dev["V"], dev["HW"])
    bound = 1e-10 * _norm(ctx, dev["W"]) * _norm(ctx, dev["HV"])
    print("<W,HV> %.16e  <V,HW> %.16e  diff %.2e  bound %.2e" % (a, b, abs(a - b), bound))
    assert abs(a - b) <= bound


def test_power_of_two_scaling_is_exact(dev):
    ctx = dev["ctx"]
    ctx.forward([dev["X"]])
    assert np.array_equal(ctx.hessvec([8. * dev["V"]])[0][0], 8. * dev["HV"])
    assert np.array_equal(ctx.hessvec([dev["V"] / 8.])[0][0], dev["HV"] / 8.)
    assert np.array_equal(ctx.hessvec([dev["V"]])[0][0], dev["HV"])


def test_central_differences_of_device_gradients(dev):
    ctx, X, V = dev["ctx"], dev["X"], dev["V"]

    def grad(Y):
        ctx.forward([Y])
        return ctx.adjoint()[0]
    err = [np.linalg.norm((grad(X + e * V) - grad(X - e * V)) / (2. * e) - dev["HV"]) for e in (1e-3, 1e-4)]
    print("FD errors", err, "ratio", err[0] / err[1])
    assert 90. <= err[0] / err[1] <= 110.


def test_third_taylor_remainder_on_device_callbacks(dev):
    ctx = dev["ctx"]
    AA = hessian.taylor_table_2(dev["X"], dev["V"], lambda Y: ctx.forward([Y]), lambda Y: ctx.adjoint()[0],
                                lambda Y, D: ctx.hessvec([D])[0][0], ctx.inner, epsilon=0.1)
    print("R3", AA[3], "slopes", AA[6, :4])
    assert np.all(np.abs(AA[6, 1:4] - 3.) <= 0.06)


# ---- (3) batch, members, horizons ---------------------------------------------------------------------------------------------------------
AVALS = (-0.3, -0.2, -0.4)
HZ = (4, 2, 3)


def _members(Npts):
    G = 2 * Npts
    xs = [synthetic_ic(G, ho.SEED_X + b, ho.E0) for b in range(3)]
    vs = [synthetic_ic(G, ho.SEED_V + 10 * b, ho.E0) for b in range(3)]
    return xs, vs


@pytest.mark.parametrize("Npts", [64, 54])
def test_members_equal_batch_one_contexts(Npts):
    xs, vs = _members(Npts)
    G = 2 * Npts
    ctx = _capi.Context(_capi.SMO_SH23, Npts, BOX, 0.1, max(HZ), AVALS)
    ctx.set_horizons(HZ)
    ctx.forward([np.concatenate(xs)])
    (HV,), dJ = ctx.hessvec([np.concatenate(vs)])
    assert HV.shape == (3 * G,) and dJ.shape == (3,)
    # device vectors: the same bits as the host form
    dX, dV, dH = DeviceVector.from_numpy(np.concatenate(xs)), DeviceVector.from_numpy(np.concatenate(vs)), DeviceVector(3 * G)
    ctx.forward_dev([dX])
    _, dJ_dev = ctx.hessvec_dev([dV], [dH])
    assert np.array_equal(dH.numpy(), HV) and np.array_equal(dJ_dev, dJ)
    out, dJ_any = ctx.hessvec_any([dV])
    assert isinstance(out[0], DeviceVector) and np.array_equal(out[0].numpy(), HV) and np.array_equal(dJ_any, dJ)
    ctx.close()
    for b in range(3):
        one = _ctx(Npts, 0.1, HZ[b], AVALS[b])
        one.forward([xs[b]])
        (H1,), d1 = one.hessvec([vs[b]])
        one.close()
        assert np.array_equal(HV[b * G:(b + 1) * G], H1), b
        assert dJ[b] == d1, b
        assert ho.rel(H1, _ref(Npts, 0.1, HZ[b], AVALS[b], (ho.SEED_X + b, ho.SEED_V + 10 * b))[3]) < RTOL
    del dX, dV, dH, out
    gc.collect()


# ---- (4) state and refusals -------------------------------------------------------------------------------------------------------------------
def test_state_rules():
    Npts, dt, N = 64, 0.1, 8
    X, V, W = ho.inputs(Npts)
    plain = _ctx(Npts, dt, N)
    plain.forward([X])
    g_plain = plain.adjoint()[0]
    plain.close()

    ctx = _ctx(Npts, dt, N)
    bytes0 = ctx.stack_bytes
    with pytest.raises(_capi.SmoError) as e:
        ctx.hessvec([V])
    assert e.value.code == 4 and "forward" in str(e.value)                     # SMO_ERR_STATE
    ctx.forward([X])
    n = _capi.C.c_size_t()
    assert _capi.lib().smo_stack_bytes(ctx._h, _capi.C.byref(n)) == 0 and n.value == bytes0      # nothing allocated before the first product
    g_before = ctx.adjoint()[0]
    (HV,), _ = ctx.hessvec([V])
    assert ctx.stack_bytes == 2 * bytes0
    (HW,), _ = ctx.hessvec([W])
    assert ctx.stack_bytes == 2 * bytes0 and not np.array_equal(HV, HW)
    g_after = ctx.adjoint()[0]
    assert np.array_equal(g_before, g_plain) and np.array_equal(g_after, g_plain)
    assert np.array_equal(ctx.hessvec([V])[0][0], HV)                           # and products stay valid after the adjoint
    assert [t["kernel"] for t in ctx.timing()][-2:] == ["sh23_tangent_kernel", "sh23_soa_kernel"]

    ctx.set_horizons([N])
    with pytest.raises(_capi.SmoError) as e:
        ctx.hessvec([V])
    assert e.value.code == 4
    ctx.forward([X])
    assert np.array_equal(ctx.hessvec([V])[0][0], HV)

    # arguments: null vectors, HV overlapping V (host form: any overlap of the two ranges)
    L, h = _capi.lib(), ctx._h
    buf = np.zeros(3 * Npts)
    v_ptr = _capi._ptr_array([buf.ctypes.data])
    assert L.smo_hessvec(h, None, v_ptr, None) == 1 and L.smo_hessvec(h, v_ptr, None, None) == 1
    assert L.smo_hessvec(h, _capi._ptr_array([None]), v_ptr, None) == 1 and L.smo_hessvec_dev(h, v_ptr, _capi._ptr_array([None]), None) == 1
    assert L.smo_hessvec(h, v_ptr, v_ptr, None) == 1 and b"overlap" in L.smo_last_error()
    assert L.smo_hessvec(h, v_ptr, _capi._ptr_array([buf.ctypes.data + 8 * Npts]), None) == 1 and b"overlap" in L.smo_last_error()
    with pytest.raises(ValueError):
        ctx.hessvec([V[:-1]])
    ctx.close()


def test_other_kinds_refuse():
    made = [
        _capi.Context(_capi.SMO_SHB23, 64, (-20., 20.), 1e-2, 2, -0.1),
        _capi.Context(_capi.SMO_KDYN, 8, (0., 2. * np.pi), 1e-2, 2, 1.),
        _capi.Context(_capi.SMO_POIS, 24, (0., 4. * np.pi), 5e-3, 2, 500., cost=0, npts2=24, param2=0.05, param3=1., param4=0.3),
    ]
    for ctx in made:
        n = ctx.vec_len
        with pytest.raises(_capi.SmoError) as e:
            ctx.hessvec([np.zeros(n)])
        assert e.value.code == 6 and "SH23" in str(e.value), ctx.cfg.kind       # SMO_ERR_UNSUPPORTED
        v, hv = np.zeros(n), np.zeros(n)
        assert _capi.lib().smo_hessvec_dev(ctx._h, _capi._ptr_array([v.ctypes.data]), _capi._ptr_array([hv.ctypes.data]), None) == 6
        ctx.close()


def test_continuous_adjoint_has_no_hessian():
    dom, X = sh23.Generate_IC(ho.E0, Npts=16)
    buf = sh23.GEN_BUFFER(dom, 3)
    sh23.FWD_Solve_IVP_Lin([X], dom, 0.1, 3, 3, buf)
    with pytest.raises(ValueError, match="Continuous"):
        sh23.HESS_Solve_IVP_Lin([X], [X], dom, 0.1, 3, 3, buf, None, "Continuous")
    HV = sh23.HESS_Solve_IVP_Lin([X], [X], dom, 0.1, 3, 3, buf, None, "Discrete")
    assert len(HV) == 1 and HV[0].shape == X.shape and np.all(np.isfinite(HV[0]))
    dom.drop_contexts()


# ---- (5) device memory contents -----------------------------------------------------------------------------------------------------------------
def _single():
    X, V, _ = ho.inputs(64)
    ctx = _ctx(64, 0.1, 40)
    ctx.forward([X])
    (HV,), dJ = ctx.hessvec([V])
    ctx.close()
    return [HV, np.asarray(dJ)]


def _batched():
    out = []
    for Npts in (64, 54):
        xs, vs = _members(Npts)
        ctx = _capi.Context(_capi.SMO_SH23, Npts, BOX, 0.1, max(HZ), AVALS)
        ctx.set_horizons(HZ)
        ctx.forward([np.concatenate(xs)])
        (HV,), dJ = ctx.hessvec([np.concatenate(vs)])
        ctx.close()
        out += [HV, dJ]
    return out


@pytest.mark.parametrize("run", [_single, _batched], ids=["64-0.1-40", "batch3-horizons"])
def test_results_do_not_depend_on_what_memory_held(run, monkeypatch):
    monkeypatch.delenv("SMO_POISON", raising=False)
    ref = run()
    assert all(np.all(np.isfinite(v)) for v in ref)
    for fill in (0, 255, 63):
        monkeypatch.setenv("SMO_POISON", str(fill))
        got = run()
        for k, (r, g) in enumerate(zip(ref, got)):
            assert np.array_equal(r, g), "SMO_POISON=%d: value %d differs" % (fill, k)
    monkeypatch.delenv("SMO_POISON")


# ---- (6) the example -------------------------------------------------------------------------------------------------------------------------------
def test_second_order_example(in_tmp_cwd):
    from spheremanopt_amd.examples import sh23_second_order
    res = sh23_second_order.main(["--npts", "16", "--n-iters", "20", "--max-iters", "3", "--k", "31", "--quiet"])
    theta, scale = res["theta"], np.max(np.abs(res["theta"]))
    print("Lanczos steps %d  theta_min %.10e  theta_max %.10e  residuals %s" % (len(theta), theta[0], theta[-1], res["residuals"]))
    assert 2 <= len(theta) <= 31 and np.all(np.isfinite(theta))
    assert max(res["residuals"]) <= 1e-9 * scale
    assert res["minimum"] == (res["descent_direction"] is None)
    # the same Lanczos run on the restatement's Hessian at the point the example stopped at
    X, E0 = res["X"], ho.E0
    o = ho.oracle(16, 0.1, 20)
    _, g, _ = ho.hessvec(o, X, res["v0"])
    op = lambda V: hessian.riemannian_hessvec(X, E0, V, g, lambda W: ho.hessvec(o, X, W)[2], o.inner)
    theta_ref, _, _ = hessian.extreme_eigs(op, res["v0"], o.inner, 31, project=lambda Z: Z - (o.inner(X, Z) / E0) * X)
    print("restatement: Lanczos steps %d  theta_min %.10e" % (len(theta_ref), theta_ref[0]))
    assert abs(theta[0] - theta_ref[0]) <= 1e-6 * abs(theta_ref[0])
    res["domain"].drop_contexts()
