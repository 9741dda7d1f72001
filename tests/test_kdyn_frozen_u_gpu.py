"""KDyn with a frozen velocity (smo_create_frozen_u): a context that computes dJ/dB0 alone.  Its yardsticks are the project's own full-gradient
context — J, dJ/dB0, <B0, dJ/dB0> and the snapshots must be EQUAL, bit for bit — and oracle/kdyn.py (1e-6, the north-star tolerance)."""
import ctypes as C
import functools

import numpy as np
import pytest

from spheremanopt_amd import _capi, kdyn
from spheremanopt_amd.devvec import DeviceVector, to_device, to_host
from spheremanopt_amd.sphere_opt import Optimise_On_Multi_Sphere
from spheremanopt_amd.test_grad import Adjoint_Gradient_Test
from test_kdyn_batch_gpu import ADJS, _equal, _members, _stack

pytestmark = pytest.mark.gpu
RM, DT = 1.3, 1e-2
RTOL = 1e-6                                    # tests/test_kdyn_gpu.py
COSTS = ("Final", "Integrated")


@functools.lru_cache(maxsize=2)
def _fields(G, count=1):
    """`count` (B0, U) pairs, computed once per grid and left unchanged (member 1 is a 'dirty' one: not solenoidal, full spectrum)."""
    return tuple(_members(G, range(1, 1 + count)))


def _solve(ctx, members, n, snaps=()):
    """forward, both adjoint types, <B0, dJ/dB0> and snapshots on one context: per member [J, {adj: (gB, last gradient)}, inner, snaps].
    (The last gradient is dJ/dU on a full context and dJ/dB0 again on a frozen one, so that _equal compares like with like.)"""
    B = len(members)
    X = _stack(members) if B > 1 else list(members[0])
    J = np.atleast_1d(ctx.forward(X))
    res = [[J[b], {}, None, None] for b in range(B)]
    for adj in ADJS:
        g = ctx.adjoint(None, adj)
        assert len(g) == (1 if ctx.frozen_u else 2)
        for b in range(B):
            res[b][1][adj] = tuple(v[b * ctx.vec_len:(b + 1) * ctx.vec_len] for v in (g[0], g[-1]))
    ip = np.atleast_1d(ctx.inner(X[0], g[0]))
    for b in range(B):
        res[b][2] = ip[b]
        res[b][3] = [ctx.snapshot(i, b) for i in snaps]
    return res


def _equal_B(a, b):
    """J, dJ/dB0 of both adjoint types, <B0, dJ/dB0> and the snapshots, bit for bit (dJ/dU is not compared)."""
    assert a[0] == b[0], (a[0], b[0])
    for adj in ADJS:
        assert np.array_equal(a[1][adj][0], b[1][adj][0]), adj
    assert a[2] == b[2], (a[2], b[2])
    assert len(a[3]) == len(b[3])
    for s, t in zip(a[3], b[3]):
        assert np.array_equal(s, t)


def _full_and_frozen(N, n, cost, members, snaps, ckpt=1, keep_states=True, Rm=RM):
    B = len(members)
    dom = kdyn.KDynDomain(N, ckpt=ckpt)
    fro = dom.context(Rm, DT, n, cost, batch=B, frozen_U=True, keep_states=keep_states)
    info = {k: fro.get(k) for k in (0, 1, 2, 6)}
    got = _solve(fro, members, n, snaps)
    info[2] = fro.get(2)
    info["stack_bytes"], info["snapshot_len"] = fro.stack_bytes, fro.snapshot_len
    dom.drop_contexts()
    dom = kdyn.KDynDomain(N)
    full = dom.context(Rm, DT, n, cost, batch=B)
    info["full6"] = full.get(6)
    ref = _solve(full, members, n, snaps)
    dom.drop_contexts()
    return got, ref, info


# (Npts, n): G = 12 smallest tuned length; 18 factor 3 twice; 30 radix 5; 42 radix 7; 36 captured graphs; 15, 33 run-time length, odd grids;
# 192 the bench shape (2 of 3 prefetched items in the full pass, full twiddle table); 240 halved tiles, half twiddle table
_SIZES = [(8, 3), (12, 3), (20, 3), (28, 3), (24, 4), (10, 3), (22, 3), (128, 2), (160, 1)]


@pytest.mark.parametrize("N,n", _SIZES)
@pytest.mark.parametrize("cost", COSTS)
def test_bit_identical_with_the_full_context(N, n, cost):
    members = _fields(3 * N // 2)
    got, ref, info = _full_and_frozen(N, n, cost, members, (0, n // 2, n))
    _equal_B(got[0], ref[0])
    assert info[6] == 1 and info["full6"] == 0 and info[1] == 0
    if N == 24:
        assert info[2] > 0                                     # G = 36: the solves were replayed from captured graphs


@pytest.mark.parametrize("N,n", [(8, 3), (16, 6)])
@pytest.mark.parametrize("cost", COSTS)
def test_against_the_oracle(N, n, cost):
    from oracle.kdyn import KDynOracle
    (B0, U), = _fields(3 * N // 2)
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(RM, DT, n, cost, frozen_U=True)
    J = ctx.forward([B0, U])
    g = {adj: ctx.adjoint(None, adj)[0] for adj in ADJS}
    dom.drop_contexts()
    o = KDynOracle(N, Rm=RM, dt=DT, N_ITERS=n, Cost_function=cost)
    Jo = o.forward([B0, U])
    print("J %.17g oracle %.17g" % (J, Jo))
    assert abs(J - Jo) <= RTOL * abs(Jo)
    for adj in ADJS:
        go = o.adjoint([B0, U], adj)[0]
        r = float(np.linalg.norm(g[adj] - go) / np.linalg.norm(go))
        print(adj, "rel err of dJ/dB0", r)
        assert r < RTOL, (adj, r)


def test_batch_with_one_Rm_per_member():
    N, n, cost, rms = 16, 3, "Final", (0.7, 1.3, 2.9)
    members = _fields(24, 3)
    got, ref, _ = _full_and_frozen(N, n, cost, members, (0, n), Rm=rms)
    for b in range(3):
        _equal_B(got[b], ref[b])                               # member b of the smo_create_members full context
        dom = kdyn.KDynDomain(N)
        one = _solve(dom.context(rms[b], DT, n, cost, frozen_U=True), [members[b]], n, (0, n))[0]
        dom.drop_contexts()
        _equal(got[b], one)                                    # a batch-1 frozen context at Rm_b
    assert len({r[0] for r in got}) == 3
    same = _full_and_frozen(N, n, cost, [members[0]] * 3, (n,), Rm=rms)[0]
    assert len({r[0] for r in same}) == 3                     # one input, three Rm: three different J


@pytest.mark.parametrize("cost", COSTS)
def test_checkpoint_windows(cost):
    N, n = 16, 5
    members = _fields(24)
    X = list(members[0])
    keep = _full_and_frozen(N, n, cost, members, (0, 3, n))[0][0]
    dom = kdyn.KDynDomain(N, ckpt=2)
    ctx = dom.context(RM, DT, n, cost, frozen_U=True)
    assert ctx.get(0) == 2 and ctx.get(1) == 0
    got = _solve(ctx, members, n, (0, 3, n))[0]
    _equal(got, keep)
    J = ctx.forward(X)
    s3 = ctx.snapshot(3)                                       # a state that is not kept: its window is recomputed ...
    g = ctx.adjoint(None, "Discrete")[0]                       # ... and the adjoint after it is still the keep-all one
    dom.drop_contexts()
    assert J == keep[0] and np.array_equal(s3, keep[3][1]) and np.array_equal(g, keep[1]["Discrete"][0])


@pytest.mark.parametrize("N,n", [(16, 5), (24, 4)])
def test_stack_free(N, n):
    members = _fields(3 * N // 2)
    got, ref, info = _full_and_frozen(N, n, "Final", members, (n,), keep_states=False)
    _equal_B(got[0], ref[0])
    assert info["stack_bytes"] == 2 * 1 * 8 * info["snapshot_len"] and info[0] == n and info[6] == 1
    if N == 24:
        assert info[2] > 0
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(RM, DT, n, "Final", frozen_U=True, keep_states=False)
    other = _members(3 * N // 2, [4])[0]
    ctx.forward(list(other))
    J = ctx.forward(list(members[0]))                          # two forwards, one adjoint: the second forward's gradient
    g = ctx.adjoint(None, "Discrete")[0]
    assert J == ref[0][0] and np.array_equal(g, ref[0][1]["Discrete"][0])
    with pytest.raises(_capi.SmoError) as e:
        ctx.snapshot(0)
    assert e.value.code == 4 and "keep_states" in str(e.value)
    dom.drop_contexts()
    with pytest.raises(_capi.SmoError) as e:
        _capi.Context(_capi.SMO_KDYN, N, (0., 2 * np.pi), DT, n, RM, cost="Integrated", frozen_u=True, keep_states=False)
    assert e.value.code == 1 and "Integrated" in str(e.value)


def test_stack_free_batch_bytes():
    dom = kdyn.KDynDomain(16)
    ctx = dom.context((0.7, 1.3, 2.9), DT, 7, "Final", frozen_U=True, keep_states=False)
    assert ctx.stack_bytes == 2 * 3 * 8 * ctx.snapshot_len
    dom.drop_contexts()


def test_second_gradient_pointer_is_never_written():
    N, n = 16, 3
    (B0, U), = _fields(24)
    L = _capi.lib()
    ctx = _capi.Context(_capi.SMO_KDYN, N, (0., 2 * np.pi), DT, n, RM, frozen_u=True)
    assert L.smo_ncomp(ctx._h) == 2
    J = ctx.forward([B0, U])
    ref = ctx.adjoint(None)[0]
    # host entry point: a sentinel-filled second buffer comes back untouched; NULL in its place is fine
    g0, g1 = np.zeros(ctx.vec_len), np.full(ctx.vec_len, -7.25)
    x = _capi._ptr_array([None, None])
    assert L.smo_adjoint(ctx._h, x, 0, _capi._ptr_array([g0.ctypes.data, g1.ctypes.data])) == 0
    assert np.array_equal(g0, ref) and np.all(g1 == -7.25)
    g0[:] = 0
    assert L.smo_adjoint(ctx._h, x, 0, _capi._ptr_array([g0.ctypes.data, None])) == 0
    assert np.array_equal(g0, ref)
    # device entry point
    d0, d1 = DeviceVector(ctx.vec_len), DeviceVector.from_numpy(g1)
    assert L.smo_adjoint_dev(ctx._h, x, 0, _capi._ptr_array([d0.ptr, d1.ptr])) == 0
    assert np.array_equal(d0.numpy(), ref) and np.all(d1.numpy() == -7.25)
    d2 = DeviceVector(ctx.vec_len)
    assert L.smo_adjoint_dev(ctx._h, x, 0, _capi._ptr_array([d2.ptr, None])) == 0
    assert np.array_equal(d2.numpy(), ref)
    assert L.smo_adjoint_dev(ctx._h, x, 0, _capi._ptr_array([None, d1.ptr])) == 1      # grad[0] is still required
    assert J == ctx.forward_dev(to_device([B0, U]))
    ctx.close()


def test_refusals():
    box = (0., 2 * np.pi)
    with pytest.raises(_capi.SmoError) as e:
        _capi.Context(_capi.SMO_KDYN, 16, box, DT, 2, RM, world=2, rank=0, frozen_u=True)
    assert e.value.code == 6
    for kind, npts, iv in ((_capi.SMO_SH23, 64, (0., 12 * np.pi)), (_capi.SMO_SHB23, 64, (-20., 20.)), (_capi.SMO_POIS, 24, (0., 4 * np.pi))):
        with pytest.raises(_capi.SmoError) as e:
            _capi.Context(kind, npts, iv, DT, 2, 1.0, npts2=24, frozen_u=True)
        assert e.value.code == 6, kind
    with pytest.raises(_capi.SmoError) as e:
        _capi.Context(_capi.SMO_KDYN, 16, box, DT, 2, (1.0, -2.0, 3.0), frozen_u=True)
    assert e.value.code == 1 and "member 1" in str(e.value)
    with pytest.raises(_capi.SmoError) as e:
        _capi.Context(_capi.SMO_KDYN, 16, box, DT, 2, (1.0, float("nan")), frozen_u=True)
    assert e.value.code == 1 and "member 1" in str(e.value)
    ctx = _capi.Context(_capi.SMO_KDYN, 16, box, DT, 2, RM, frozen_u=True)
    assert _capi.lib().smo_kdyn_op(ctx._h, _capi.SMO_KD_SYNC, 0, 0, None, None, None) == 6
    with pytest.raises(ValueError):
        ctx.adjoint_dev(None, [DeviceVector(ctx.vec_len), DeviceVector(ctx.vec_len)])      # the binding hands out ONE gradient
    ctx.close()


def test_taylor_remainder_one_sphere(in_tmp_cwd):
    """test_kdyn_gpu.py's Taylor test (N = 16, n = 10, dt = 1e-2, eps = 1e-3, |slope - 2| < 5e-3) with the velocity frozen."""
    N, n, dt = 16, 10, 1e-2
    dom = kdyn.KDynDomain(N)
    B0 = kdyn.synthetic_field(dom.G, 1) + 0.2 * np.random.RandomState(9).standard_normal(dom.vec_len) + 0.05
    U = kdyn.synthetic_field(dom.G, 2) + 0.2 * np.random.RandomState(10).standard_normal(dom.vec_len)
    dom.freeze_velocity(U)
    buf = kdyn.GEN_BUFFER(N, dom, n)
    args_f = [dom, 1., dt, n, n, buf, "Final", "Discrete"]
    AA = Adjoint_Gradient_Test([B0], [kdyn.synthetic_field(dom.G, 3)], kdyn.FWD_Solve_IVP_Lin_B, kdyn.ADJ_Solve_IVP_Lin_B, kdyn.Inner_Prod_3,
                               args_f, (dom, None), epsilon=1e-3)
    dom.drop_contexts()
    print(AA)
    assert np.all(np.abs(AA[4, :4] - 2.0) < 5e-3), AA


def test_optimiser_trace_equals_the_full_context_with_U_held_fixed(in_tmp_cwd):
    N, n = 8, 4
    (B0, U), = _fields(12)
    B0 = B0 / np.sqrt(np.mean(B0.reshape(3, -1) ** 2, axis=1).sum())           # <B0,B0> = 1
    runs = []
    for frozen in (True, False):
        dom = kdyn.KDynDomain(N)
        buf = kdyn.GEN_BUFFER(N, dom, n)
        args_f = [dom, RM, DT, n, n, buf, "Final", "Discrete"]
        if frozen:
            dom.freeze_velocity(U)
            f, g = kdyn.FWD_Solve_IVP_Lin_B, kdyn.ADJ_Solve_IVP_Lin_B
        else:
            def f(X, *a):
                return kdyn.FWD_Solve_IVP_Lin([X[0], U], *a)

            def g(X, *a):
                return kdyn.ADJ_Solve_IVP_Lin([X[0], U], *a)[:1]
        R, F, X = Optimise_On_Multi_Sphere([B0.copy()], [1.], f, g, kdyn.Inner_Prod_3, args_f, (dom, None), max_iters=4, alpha_k=10.,
                                           LS='LS_wolfe', CG=True, verbose=False)
        runs.append((R, F, X[0]))
        dom.drop_contexts()
    assert len(runs[0][1]) >= 2
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and np.array_equal(runs[0][2], runs[1][2])


def test_example_runs_to_the_end(in_tmp_cwd):
    from spheremanopt_amd.examples import kdyn_seed_field
    R, F, X = kdyn_seed_field.main(["--npts", "24", "--dt", "5e-4", "--steps", "40", "--max-iters", "3", "--quiet"])
    assert len(F) == 3 and F[-1] > F[0] > 0
    x = to_host(X)
    assert len(x) == 1 and x[0].shape == (3 * 36 ** 3,)
    R2, F2, _ = kdyn_seed_field.main(["--npts", "24", "--dt", "5e-4", "--steps", "40", "--max-iters", "3", "--quiet", "--no-states"])
    assert F2 == F
