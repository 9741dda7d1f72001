"""KDyn members with a time horizon of their own (smo_set_horizons).  The yardstick is the project's strongest: member b of a context whose
horizons are N_b must equal, BIT FOR BIT, a batch-1 context created with n_iters = N_b on member b's input — J, both gradients, both adjoint
types, both costs, <x_b, y_b> and the snapshots at member times — with and without captured graphs, checkpoint windows, a frozen velocity, one
Rm per member, and on the run-time-length kernels.  One case is held against oracle/kdyn.py at the project's 1e-6."""
import functools

import numpy as np
import pytest

from spheremanopt_amd import _capi, kdyn
from spheremanopt_amd.devvec import DeviceVector, to_device
from test_kdyn_batch_gpu import ADJS, _equal, _members, _stack

pytestmark = pytest.mark.gpu
RM, DT = 1.3, 1e-2
BOX = (0., 2 * np.pi)
COSTS = ("Final", "Integrated")
HZ5 = (6, 1, 3, 2, 6)                          # horizon 1, the capacity itself, a repeated value


@functools.lru_cache(maxsize=None)
def _fields(G, count):
    """`count` (B0, U) pairs per grid, made once and left unchanged (odd members are 'dirty': not solenoidal, full spectrum)."""
    return tuple(_members(G, range(count)))


def _times(nb):
    return (0, nb // 2, nb)


def _solve(ctx, members, hz, times=_times):
    """forward, both adjoint types, <B0, last gradient> and the snapshots at member times on one context: per member
    [J, {adj: (gB, last gradient)}, inner, snaps] (the last gradient is dJ/dU, or dJ/dB0 again on a frozen-velocity context)."""
    B = len(members)
    X = _stack(members) if B > 1 else list(members[0])
    J = np.atleast_1d(ctx.forward(X))
    res = [[J[b], {}, None, None] for b in range(B)]
    for adj in ADJS:
        g = ctx.adjoint(None, adj)
        for b in range(B):
            res[b][1][adj] = tuple(v[b * ctx.vec_len:(b + 1) * ctx.vec_len] for v in (g[0], g[-1]))
    ip = np.atleast_1d(ctx.inner(X[0], g[-1]))
    for b in range(B):
        res[b][2] = ip[b]
        res[b][3] = [ctx.snapshot(i, b) for i in times(hz[b])]
    return res


@functools.lru_cache(maxsize=None)
def _single(N, count, b, nb, cost, rm=RM, frozen=False, keep=True, times=_times):
    """Member b alone on a keep-all batch-1 context created with n_iters = nb: the reference of every comparison, computed once."""
    dom = kdyn.KDynDomain(N)
    kw = dict(frozen_U=True, keep_states=keep) if frozen else {}
    res = _solve(dom.context(rm, DT, nb, cost, **kw), [_fields(3 * N // 2, count)[b]], [nb], times)[0]
    dom.drop_contexts()
    return res


def _check(got, N, count, hz, cost, rms=None, **kw):
    for b, nb in enumerate(hz):
        _equal(got[b], _single(N, count, b, nb, cost, rm=RM if rms is None else rms[b], **kw))


# N = 16: G = 24, tuned;  N = 24: G = 36, tuned, captured graphs;  N = 22: G = 33, run-time-length kernels, odd grid
@pytest.mark.parametrize("N,hz", [(16, HZ5), (24, HZ5), (22, (5, 1, 3))])
@pytest.mark.parametrize("cost", COSTS)
def test_members_equal_batch_one_contexts_of_their_own_horizon(N, hz, cost):
    members = _fields(3 * N // 2, len(hz))
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(RM, DT, hz, cost)
    assert ctx.horizons == tuple(hz) and ctx.batch == len(hz) and ctx.cfg.n_iters == max(hz)
    got = _solve(ctx, members, hz)
    replays = ctx.get(2)
    out = (_capi.C.c_int * len(hz))()
    assert _capi.lib().smo_get_horizons(ctx._h, out) == 0 and tuple(out) == tuple(hz)
    dom.drop_contexts()
    assert replays > 0 or N != 24                                  # G = 36: the solves were replayed from captured graphs
    _check(got, N, len(hz), hz, cost)
    assert len({r[0] for r in got}) == len(hz)                    # (members 0 and 4 share a horizon, not an input)


@pytest.mark.parametrize("keep", [True, False])
def test_frozen_velocity_with_one_Rm_per_member(keep):
    N, hz, rms, cost = 16, (4, 1, 3), (0.7, 1.3, 2.9), "Final"
    members = _fields(24, 3)
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(rms, DT, hz, cost, frozen_U=True, keep_states=keep)
    assert ctx.frozen_u and ctx.params == rms and ctx.horizons == hz
    times = _times if keep else (lambda nb: (nb,))
    got = _solve(ctx, members, hz, times)
    if not keep:
        with pytest.raises(_capi.SmoError) as e:
            ctx.snapshot(0, 1)                                     # only the member's last state is held
        assert e.value.code == 4
    dom.drop_contexts()
    _check(got, N, 3, hz, cost, rms=rms, frozen=True, keep=keep, times=times)


@pytest.mark.parametrize("cost", COSTS)
def test_frozen_velocity_keeping_states(cost):
    N, hz = 16, (5, 2, 5, 1)
    dom = kdyn.KDynDomain(N)
    got = _solve(dom.context(RM, DT, hz, cost, frozen_U=True), _fields(24, 4), hz)
    dom.drop_contexts()
    _check(got, N, 4, hz, cost, frozen=True)


def _times7(nb):
    """Capacity 7: member times whose states lie inside a recomputed window and below a checkpoint (state = 7 - nb + i)."""
    return tuple(sorted({0, 1, nb // 2, nb - 1, nb}))


@pytest.mark.parametrize("ckpt", [2, 3])
def test_checkpoint_windows(ckpt):
    N, hz, cost = 16, (7, 1, 4, 2, 5), "Integrated"
    dom = kdyn.KDynDomain(N, ckpt=ckpt)
    ctx = dom.context(RM, DT, hz, cost)
    assert ctx.get(0) == ckpt
    got = _solve(ctx, _fields(24, 5), hz, _times7)
    # a snapshot read that replays a window, then the adjoint: still the keep-all one
    s = ctx.snapshot(2, 2)                                         # member 2 (first state 3): state 5, inside a window, below the checkpoint 6
    g = ctx.adjoint(None, "Discrete")
    dom.drop_contexts()
    _check(got, N, 5, hz, cost, times=_times7)                       # against keep-all batch-1 runs
    ref = _single(N, 5, 2, 4, cost, times=_times7)
    assert np.array_equal(s, ref[3][2])
    L = 3 * 24 ** 3
    assert np.array_equal(g[0][2 * L:3 * L], ref[1]["Discrete"][0]) and np.array_equal(g[1][2 * L:3 * L], ref[1]["Discrete"][1])


def test_new_horizons_keep_the_captured_graphs():
    N, cost, B = 24, "Final", 3
    members = _fields(36, 5)[:B]
    ctx = _capi.Context(_capi.SMO_KDYN, N, BOX, DT, 6, RM, cost=cost, batch=B)
    plain = _solve(ctx, members, (6,) * B)                          # no table: the plain batch, captured once
    r0 = ctx.get(2)
    assert r0 > 0 and ctx.horizons is None
    for hz in ((6, 1, 3), (2, 6, 4)):
        ctx.set_horizons(hz)
        got = _solve(ctx, members, hz)
        _check(got, N, 5, hz, cost)
    r1 = ctx.get(2)
    ctx.set_horizons((3, 3, 5))                                     # new values in the table: the graphs of (6, 1, 3) go on being replayed
    got = _solve(ctx, members, (3, 3, 5))
    assert ctx.get(2) - r1 == 3                                     # one forward, two adjoint types: three replays, no capture in between
    _check(got, N, 5, (3, 3, 5), cost)
    ctx.set_horizons(None)
    assert ctx.horizons is None
    again = _solve(ctx, members, (6,) * B)
    ctx.close()
    for a, b in zip(again, plain):
        _equal(a, b)
    _check(again, N, 5, (6,) * B, cost)


@pytest.mark.parametrize("var,val", [("SMO_KD_GRAPH", "0"), ("SMO_KD_FUSE_NEXT", "0"), ("SMO_KD_ADJ_SEQ", "0"), ("SMO_KD_ANY", "1")])
def test_environment_variants(monkeypatch, var, val):
    N, hz, cost = 24, (5, 1, 3), "Integrated"
    refs = [_single(N, 3, b, nb, cost) for b, nb in enumerate(hz)]      # (the default build of the reference, made before the switch)
    monkeypatch.setenv(var, val)
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(RM, DT, hz, cost)
    got = _solve(ctx, _fields(36, 3), hz)
    replays = ctx.get(2)
    dom.drop_contexts()
    assert (replays == 0) == (var == "SMO_KD_GRAPH")
    if var in ("SMO_KD_GRAPH", "SMO_KD_FUSE_NEXT"):                  # same kernels per element: the bits of the default path
        for a, b in zip(got, refs):
            _equal(a, b)
    # ... and every variant equals batch-1 contexts of the same variant
    for b, nb in enumerate(hz):
        dom = kdyn.KDynDomain(N)
        one = _solve(dom.context(RM, DT, nb, cost), [_fields(36, 3)[b]], [nb])[0]
        dom.drop_contexts()
        _equal(got[b], one)


def test_uniform_table_gives_the_bits_of_the_plain_batch():
    N, n, cost, B = 16, 4, "Integrated", 3
    members = _fields(24, B)
    dom = kdyn.KDynDomain(N)
    plain = _solve(dom.context(RM, DT, n, cost, batch=B), members, (n,) * B)
    table = _solve(dom.context(RM, DT, (n,) * B, cost), members, (n,) * B)
    dom.drop_contexts()
    for a, b in zip(table, plain):
        _equal(a, b)


def test_device_resident_vectors_match_the_host_path():
    N, hz, cost = 16, (4, 2, 3), "Integrated"
    X = _stack(_fields(24, 3))
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(RM, DT, hz, cost)
    J = ctx.forward(X)
    gh = ctx.adjoint(None, "Continuous")
    iph = ctx.inner(X[0], gh[1])
    Xd = to_device(X)
    gd = [DeviceVector(3 * ctx.vec_len), DeviceVector(3 * ctx.vec_len)]
    Jd = ctx.forward_dev(Xd)
    ctx.adjoint_dev(Xd, gd, "Continuous")
    ipd = ctx.inner_dev(Xd[0], gd[1])
    dom.drop_contexts()
    assert np.array_equal(J, Jd) and np.array_equal(iph, ipd)
    assert np.array_equal(gh[0], gd[0].numpy()) and np.array_equal(gh[1], gd[1].numpy())
    assert J[1] == _single(N, 3, 1, 2, cost)[0]


@pytest.mark.parametrize("cost", COSTS)
def test_a_batch_one_context_shortened(cost):
    N = 16
    ctx = _capi.Context(_capi.SMO_KDYN, N, BOX, DT, 6, RM, cost=cost)
    stack6 = ctx.stack_bytes
    ctx.set_horizons([3])
    got = _solve(ctx, _fields(24, 5)[:1], (3,))[0]
    n = _capi.C.c_size_t()
    assert _capi.lib().smo_stack_bytes(ctx._h, _capi.C.byref(n)) == 0 and n.value == stack6      # the capacity does not change
    ctx.close()
    _equal(got, _single(N, 5, 0, 3, cost))


def test_state_and_refusals():
    L = _capi.lib()
    ctx = _capi.Context(_capi.SMO_KDYN, 16, BOX, DT, 4, RM, batch=3)
    X = _stack(_fields(24, 3))
    ctx.forward(X)
    ctx.set_horizons((4, 2, 3))
    with pytest.raises(_capi.SmoError) as e:
        ctx.adjoint(None)                                           # the setter cleared the forward state
    assert e.value.code == 4
    ctx.forward(X)
    ctx.snapshot(2, 1)
    with pytest.raises(_capi.SmoError) as e:
        ctx.snapshot(3, 1)                                          # member 1 has states 0 .. 2
    assert e.value.code == 1
    for bad in ((4, 0, 3), (4, 2, 5)):
        with pytest.raises(_capi.SmoError) as e:
            ctx.set_horizons(bad)
        assert e.value.code == 1 and "member %d" % (1 if bad[1] == 0 else 2) in str(e.value)
    assert ctx.horizons == (4, 2, 3)
    with pytest.raises(ValueError):
        ctx.set_horizons((4, 2))
    ctx.close()
    one = _capi.Context(_capi.SMO_KDYN, 16, BOX, DT, 4, RM)
    one.set_horizons((2,))
    assert L.smo_kdyn_op(one._h, _capi.SMO_KD_SYNC, 0, 0, None, None, None) == 6
    one.set_horizons(None)
    assert L.smo_kdyn_op(one._h, _capi.SMO_KD_SYNC, 0, 0, None, None, None) == 0
    one.close()
    two = (_capi.C.c_int * 1)(2)
    for kind, npts, iv, kw in ((_capi.SMO_SHB23, 64, (-20., 20.), {}), (_capi.SMO_POIS, 24, (0., 4 * np.pi), dict(npts2=24, param2=0.05)),
                               (_capi.SMO_KDYN, 16, BOX, dict(world=2, rank=0))):
        c = _capi.Context(kind, npts, iv, DT, 4, 500. if kind == _capi.SMO_POIS else 1.0, **kw)
        assert L.smo_set_horizons(c._h, two) == 6, kind
        assert L.smo_set_horizons(c._h, None) == 6, kind
        c.close()


def test_against_the_oracle():
    from oracle.kdyn import KDynOracle
    N, hz, b = 16, (6, 2, 4), 2
    members = _fields(24, 3)
    for cost in COSTS:
        dom = kdyn.KDynDomain(N)
        ctx = dom.context(RM, DT, hz, cost)
        J = ctx.forward(_stack(members))
        g = ctx.adjoint(None, "Discrete")
        dom.drop_contexts()
        o = KDynOracle(N, Rm=RM, dt=DT, N_ITERS=hz[b], Cost_function=cost)
        B0, U = members[b]
        Jo = o.forward([B0, U])
        goB, goU = o.adjoint([B0, U], "Discrete")
        L = 3 * 24 ** 3
        rel = lambda x, y: float(np.linalg.norm(x - y) / np.linalg.norm(y))   # noqa: E731
        print(cost, J[b], Jo, rel(g[0][b * L:(b + 1) * L], goB), rel(g[1][b * L:(b + 1) * L], goU))
        assert abs(J[b] - Jo) <= 1e-6 * abs(Jo)
        assert rel(g[0][b * L:(b + 1) * L], goB) < 1e-6 and rel(g[1][b * L:(b + 1) * L], goU) < 1e-6
