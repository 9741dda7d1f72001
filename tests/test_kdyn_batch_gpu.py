"""Batched KDyn (smo_config.batch = B > 1): B independent problems per call on one GPU.  Member b of a batch must equal, bit for bit, a
batch-1 solve of member b's inputs — J, both gradients, <x_b, y_b> and every snapshot — on the tuned and the run-time-length kernels, with
and without checkpoint windows and HIP-graph replay."""
import ctypes as C

import numpy as np
import pytest

from spheremanopt_amd import _capi, kdyn
from spheremanopt_amd.devvec import DeviceVector, to_device

pytestmark = pytest.mark.gpu
RM, DT = 1.3, 1e-2
ADJS = ("Discrete", "Continuous")


def _members(G, seeds):
    """One (B0, U) pair per seed; odd seeds get the 'dirty' treatment of test_kdyn_gpu._fields (not solenoidal, non-zero mean, full spectrum)."""
    out = []
    for s in seeds:
        B, U = kdyn.synthetic_field(G, 10 + s, 0.5 + 0.25 * s), kdyn.synthetic_field(G, 40 + s)
        if s % 2:
            rs = np.random.RandomState(70 + s)
            B = B + 0.2 * rs.standard_normal(B.size) + 0.05
            U = U + 0.2 * rs.standard_normal(U.size)
        out.append((B, U))
    return out


def _stack(members):
    return [np.concatenate([m[0] for m in members]), np.concatenate([m[1] for m in members])]


def _solve(dom, members, n, cost, snaps, batch):
    """forward, both adjoint types, inner and snapshots of `members` on ONE context of `batch` members: per member (J, {adj: (gB, gU)}, inner, snaps)."""
    B = len(members)
    ctx = dom.context(RM, DT, n, cost, batch=batch)
    X = _stack(members) if batch > 1 else list(members[0])
    J = np.atleast_1d(ctx.forward(X))
    res = [[J[b], {}, None, None] for b in range(B)]
    for adj in ADJS:
        g = ctx.adjoint(None, adj)
        for b in range(B):
            res[b][1][adj] = tuple(v[b * ctx.vec_len:(b + 1) * ctx.vec_len] for v in g)
    ip = np.atleast_1d(ctx.inner(X[0], g[0]))                       # <B0_b, dJ/dU_b> (the last adjoint type)
    for b in range(B):
        res[b][2] = ip[b]
        res[b][3] = [ctx.snapshot(i, b) for i in snaps]
    return res


def _singles(N, members, n, cost, snaps, ckpt=1):
    out = []
    for m in members:
        dom = kdyn.KDynDomain(N, ckpt=ckpt)
        out.append(_solve(dom, [m], n, cost, snaps, 1)[0])
        dom.drop_contexts()
    return out


def _equal(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for adj in ADJS:
        assert np.array_equal(a[1][adj][0], b[1][adj][0]) and np.array_equal(a[1][adj][1], b[1][adj][1]), adj
    assert a[2] == b[2], (a[2], b[2])
    for s, t in zip(a[3], b[3]):
        assert np.array_equal(s, t)


def _batched(N, members, n, cost, snaps, ckpt=1):
    dom = kdyn.KDynDomain(N, ckpt=ckpt)
    res = _solve(dom, members, n, cost, snaps, len(members))
    dom.drop_contexts()
    return res


# N = 16: G = 24, tuned;  N = 24: G = 36, tuned, captured HIP graphs;  N = 22: G = 33, run-time-length kernels, odd grid (odd vector length)
@pytest.mark.parametrize("N,B,n", [(16, 4, 3), (24, 3, 4), (22, 3, 3)])
@pytest.mark.parametrize("cost", ["Final", "Integrated"])
def test_members_equal_batch_one_runs(N, B, n, cost):
    members = _members(3 * N // 2, range(B))
    snaps = (0, n // 2, n)
    got = _batched(N, members, n, cost, snaps)
    for b, ref in enumerate(_singles(N, members, n, cost, snaps)):
        _equal(got[b], ref)
    assert len({r[0] for r in got}) == B                         # the members really differ


@pytest.mark.parametrize("ckpt", [2, 0])
def test_checkpoint_windows_are_bit_identical(ckpt):
    N, n, cost = 16, 5, "Integrated"
    members = _members(24, range(3))
    snaps = (0, 1, n // 2, n)                                     # 1: inside a recomputed window at ckpt = 2
    got = _batched(N, members, n, cost, snaps, ckpt=ckpt)
    for b, ref in enumerate(_singles(N, members, n, cost, snaps)):   # against keep-all batch-1 runs
        _equal(got[b], ref)


def test_graph_replay_off_and_on_are_bit_identical(monkeypatch):
    N, n, cost = 24, 4, "Final"
    members = _members(36, range(3))
    snaps = (0, n // 2, n)
    monkeypatch.setenv("SMO_KD_GRAPH", "0")
    off = _batched(N, members, n, cost, snaps)
    monkeypatch.delenv("SMO_KD_GRAPH")
    dom = kdyn.KDynDomain(N)
    on = _solve(dom, members, n, cost, snaps, 3)
    assert dom.context(RM, DT, n, cost, batch=3).get(2) > 0        # the default path at G = 36 did replay graphs
    dom.drop_contexts()
    for a, b in zip(off, on):
        _equal(a, b)


def test_runtime_length_kernels_at_a_tuned_size(monkeypatch):
    monkeypatch.setenv("SMO_KD_ANY", "1")
    N, n, cost = 16, 3, "Final"
    members = _members(24, range(3))
    snaps = (0, n)
    got = _batched(N, members, n, cost, snaps)
    for b, ref in enumerate(_singles(N, members, n, cost, snaps)):
        _equal(got[b], ref)


def test_permuting_members_permutes_outputs():
    N, n, cost = 16, 3, "Integrated"
    members = _members(24, range(3))
    perm = [2, 0, 1]
    a = _batched(N, members, n, cost, (n,))
    b = _batched(N, [members[p] for p in perm], n, cost, (n,))
    for i, p in enumerate(perm):
        _equal(b[i], a[p])


def test_zero_member_next_to_nonzero_ones():
    N, n, cost = 16, 3, "Final"
    G = 24
    m = _members(G, range(2))
    zero = (np.zeros(3 * G ** 3), np.zeros(3 * G ** 3))
    got = _batched(N, [m[0], zero, m[1]], n, cost, (0, n))
    ref = _singles(N, [zero], n, cost, (0, n))[0]
    _equal(got[1], ref)
    assert got[1][0] == 0.0 and not np.any(got[1][1]["Discrete"][0]) and got[0][0] != 0.0


def test_replays_see_their_own_inputs():
    """A second forward on the same (graph-replaying, G = 36) batched context with new inputs gives the new inputs' results."""
    N, n, cost = 24, 3, "Final"
    m1, m2 = _members(36, range(3)), _members(36, range(3, 6))
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(RM, DT, n, cost, batch=3)
    J1 = ctx.forward(_stack(m1))
    g1 = ctx.adjoint(None)
    J2 = ctx.forward(_stack(m2))
    g2 = ctx.adjoint(None)
    J1b = ctx.forward(_stack(m1))
    assert ctx.get(2) > 0
    dom.drop_contexts()
    assert not np.array_equal(J1, J2) and np.array_equal(J1, J1b)
    ref = _singles(N, m2, n, cost, (n,))
    for b in range(3):
        assert J2[b] == ref[b][0]
        assert np.array_equal(g2[0][b * 3 * 36 ** 3:(b + 1) * 3 * 36 ** 3], ref[b][1]["Discrete"][0])
    assert not np.array_equal(g1[0], g2[0])


def test_device_resident_vectors_match_the_host_path():
    N, n, cost, B = 16, 3, "Integrated", 3
    members = _members(24, range(B))
    X = _stack(members)
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(RM, DT, n, cost, batch=B)
    J = ctx.forward(X)
    gh = ctx.adjoint(None, "Continuous")
    iph = ctx.inner(X[0], gh[1])
    Xd = to_device(X)
    gd = [DeviceVector(B * ctx.vec_len), DeviceVector(B * ctx.vec_len)]
    Jd = ctx.forward_dev(Xd)
    ctx.adjoint_dev(Xd, gd, "Continuous")
    ipd = ctx.inner_dev(Xd[0], gd[1])
    dom.drop_contexts()
    assert np.array_equal(J, Jd) and np.array_equal(iph, ipd)
    assert np.array_equal(gh[0], gd[0].numpy()) and np.array_equal(gh[1], gd[1].numpy())


def test_stack_and_timing_bytes_scale_with_the_batch():
    N, n, B = 16, 4, 3
    dom = kdyn.KDynDomain(N)
    c1 = dom.context(RM, DT, n, "Integrated")
    cb = dom.context(RM, DT, n, "Integrated", batch=B)
    # the optional y-side stack (smo_get key 1) is off for batch > 1
    assert cb.get(1) == 0 and cb.stack_bytes == B * (c1.stack_bytes - c1.get(1))
    assert cb.vec_len == c1.vec_len and cb.snapshot_len == c1.snapshot_len
    t1, tb = c1.timing(), cb.timing()                               # (per-launch figures: fixed at context creation)
    dom.drop_contexts()
    assert [r["kernel"] for r in t1] == [r["kernel"] for r in tb]
    for r1, rb in zip(t1, tb):
        assert rb["bytes_per_launch"] == pytest.approx(B * r1["bytes_per_launch"], rel=1e-12, abs=0)
        assert rb["hbm_bytes_per_launch"] == pytest.approx(B * r1["hbm_bytes_per_launch"], rel=1e-12, abs=0)


def test_errors():
    args = (_capi.SMO_KDYN, 16, (0., 2 * np.pi), 1e-2, 2, 1.0)
    with pytest.raises(_capi.SmoError) as e:
        _capi.Context(*args, batch=0)
    assert e.value.code == 1
    with pytest.raises(_capi.SmoError) as e:
        _capi.Context(*args, batch=2, world=2, rank=0)
    assert e.value.code == 1
    cfg = _capi.smo_config(_capi.SMO_KDYN, 16, 0., 2 * np.pi, 1e-2, 2, 1.0, 0, 2, 0, 0, 1, 1, 0, 0., 0., 0.)
    h = C.c_void_p()
    assert _capi.lib().smo_create_multi(C.byref(cfg), 2, (C.c_int * 2)(0, 0), C.byref(h)) == 1 and not h.value
    ctx = _capi.Context(*args, batch=2)
    with pytest.raises(_capi.SmoError) as e:
        ctx.transform(0, np.zeros(ctx.vec_len))
    assert e.value.code == 6
    assert _capi.lib().smo_kdyn_op(ctx._h, 0, 0, 0, None, None, None) == 6
    one = np.zeros(ctx.vec_len)
    with pytest.raises(ValueError):
        ctx.forward([one, one])                                      # one member's vectors on a batch-2 context
    with pytest.raises(ValueError):
        ctx.forward_dev([DeviceVector(ctx.vec_len), DeviceVector(ctx.vec_len)])
    with pytest.raises(ValueError):
        ctx.inner(one, one)
    ctx.close()


def test_one_member_against_the_oracle():
    from oracle.kdyn import KDynOracle
    N, n, cost, adj = 16, 3, "Integrated", "Continuous"
    members = _members(24, range(3))
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(RM, DT, n, cost, batch=3)
    J = ctx.forward(_stack(members))
    g = ctx.adjoint(None, adj)
    dom.drop_contexts()
    o = KDynOracle(N, Rm=RM, dt=DT, N_ITERS=n, Cost_function=cost)
    B, U = members[2]
    Jo = o.forward([B, U]); goB, goU = o.adjoint([B, U], adj)
    L = 3 * 24 ** 3
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))   # noqa: E731
    assert abs(J[2] - Jo) <= 1e-6 * abs(Jo)
    assert rel(g[0][2 * L:], goB) < 1e-6 and rel(g[1][2 * L:], goU) < 1e-6
