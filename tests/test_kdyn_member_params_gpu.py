"""KDyn members with their own Rm (smo_create_members, KDynDomain.context(Rm=[...])): member b must equal, bit for bit, a batch-1 context of
Rm_b on member b's inputs — J, both gradients of both adjoint types, <x_b, g_b> and the snapshots — on the tuned and the run-time-length
kernels, with and without checkpoint windows and HIP-graph replay; a uniform table must give the bits of the smo_create batch.
(tests/test_member_params_cpu.py shows on the oracle that these Rm move J by > 1e-2 relative: ignoring the table cannot pass.)"""
import ctypes as C
import itertools

import numpy as np
import pytest

from spheremanopt_amd import _capi, kdyn
from spheremanopt_amd.devvec import DeviceVector, to_device
from test_kdyn_batch_gpu import ADJS, _equal, _members, _stack

pytestmark = pytest.mark.gpu
RMS, DT = (0.7, 1.3, 2.9), 1e-2


def _solve(dom, Rm, members, n, cost, snaps):
    """forward, both adjoint types, inner and snapshots on ONE context: Rm a float -> the batch-1 smo_create context on members[0], a
    sequence -> the members context.  Per member (J, {adj: (gB, gU)}, inner, snaps), the layout of test_kdyn_batch_gpu._solve."""
    ctx = dom.context(Rm, DT, n, cost)
    B = ctx.batch
    assert B == len(members) and ctx.params == (None if np.ndim(Rm) == 0 else tuple(Rm))
    X = _stack(members) if B > 1 else list(members[0])
    J = np.atleast_1d(ctx.forward(X))
    res = [[J[b], {}, None, None] for b in range(B)]
    for adj in ADJS:
        g = ctx.adjoint(None, adj)
        for b in range(B):
            res[b][1][adj] = tuple(v[b * ctx.vec_len:(b + 1) * ctx.vec_len] for v in g)
    ip = np.atleast_1d(ctx.inner(X[0], g[0]))
    for b in range(B):
        res[b][2] = ip[b]
        res[b][3] = [ctx.snapshot(i, b) for i in snaps]
    return res


def _batched(N, Rms, members, n, cost, snaps, ckpt=1):
    dom = kdyn.KDynDomain(N, ckpt=ckpt)
    res = _solve(dom, tuple(Rms), members, n, cost, snaps)
    dom.drop_contexts()
    return res


def _singles(N, Rms, members, n, cost, snaps, ckpt=1):
    out = []
    for rm, m in zip(Rms, members):
        dom = kdyn.KDynDomain(N, ckpt=ckpt)
        out.append(_solve(dom, float(rm), [m], n, cost, snaps)[0])
        dom.drop_contexts()
    return out


# N = 16: G = 24, tuned;  N = 24: G = 36, tuned, captured HIP graphs;  N = 22: G = 33, run-time-length kernels, odd grid
@pytest.mark.parametrize("N,B,n", [(16, 3, 3), (24, 3, 4), (22, 3, 3)])
@pytest.mark.parametrize("cost", ["Final", "Integrated"])
@pytest.mark.parametrize("same_input", [False, True])
def test_members_equal_batch_one_contexts_of_their_own_rm(N, B, n, cost, same_input):
    G = 3 * N // 2
    members = _members(G, [1] * B if same_input else range(B))
    snaps = (0, n // 2, n)
    dom = kdyn.KDynDomain(N)
    got = _solve(dom, RMS, members, n, cost, snaps)
    if N == 24:
        assert dom.context(RMS, DT, n, cost).get(2) > 0             # G = 36 did replay captured graphs
    dom.drop_contexts()
    for b, ref in enumerate(_singles(N, RMS, members, n, cost, snaps)):
        _equal(got[b], ref)
    for a, b in itertools.combinations([r[0] for r in got], 2):     # same input or not: the three J differ
        assert a != b
    if same_input:
        assert not np.array_equal(got[0][3][-1], got[1][3][-1]) and not np.array_equal(got[1][3][-1], got[2][3][-1])


@pytest.mark.parametrize("cost", ["Final", "Integrated"])
def test_uniform_table_equals_the_shared_parameter_batch(cost):
    N, n, snaps = 16, 3, (0, 1, 3)
    members = _members(24, range(3))
    got = _batched(N, [1.3] * 3, members, n, cost, snaps)
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(1.3, DT, n, cost, batch=3)
    X = _stack(members)
    J = ctx.forward(X)
    g = {adj: ctx.adjoint(None, adj) for adj in ADJS}
    ip = ctx.inner(X[0], g[ADJS[-1]][0])
    L = ctx.vec_len
    ref = [[J[b], {adj: tuple(v[b * L:(b + 1) * L] for v in g[adj]) for adj in ADJS}, ip[b], [ctx.snapshot(i, b) for i in snaps]] for b in range(3)]
    dom.drop_contexts()
    for a, b in zip(got, ref):
        _equal(a, b)


def test_one_member_is_the_plain_context():
    N, n, cost, snaps = 16, 3, "Integrated", (0, 3)
    m = _members(24, [1])
    got = _batched(N, [2.9], m, n, cost, snaps)
    _equal(got[0], _singles(N, [2.9], m, n, cost, snaps)[0])


@pytest.mark.parametrize("cost", ["Final", "Integrated"])
def test_every_member_against_the_oracle_of_its_rm(cost):
    from oracle.kdyn import KDynOracle
    N, n = 16, 3
    members = _members(24, range(3))
    got = _batched(N, RMS, members, n, cost, ())
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))   # noqa: E731
    for b, (rm, (B0, U)) in enumerate(zip(RMS, members)):
        o = KDynOracle(N, Rm=rm, dt=DT, N_ITERS=n, Cost_function=cost)
        Jo = o.forward([B0, U]); goB, goU = o.adjoint([B0, U], "Discrete")
        gB, gU = got[b][1]["Discrete"]
        print("member %d Rm %.1f: J %.3e gB %.3e gU %.3e" % (b, rm, abs(got[b][0] - Jo) / abs(Jo), rel(gB, goB), rel(gU, goU)))
        assert abs(got[b][0] - Jo) <= 1e-6 * abs(Jo), (b, got[b][0], Jo)
        assert rel(gB, goB) < 1e-6 and rel(gU, goU) < 1e-6, (b, rel(gB, goB), rel(gU, goU))


@pytest.mark.parametrize("ckpt", [2, 0])
def test_checkpoint_windows_are_bit_identical(ckpt):
    N, n, cost = 16, 5, "Integrated"
    members = _members(24, range(3))
    snaps = (0, 1, n // 2, n)                                     # 1: inside a recomputed window at ckpt = 2
    got = _batched(N, RMS, members, n, cost, snaps, ckpt=ckpt)
    for a, b in zip(got, _batched(N, RMS, members, n, cost, snaps)):  # against keep-all
        _equal(a, b)


def test_graph_replay_off_and_on_are_bit_identical(monkeypatch):
    N, n, cost = 24, 4, "Final"
    members = _members(36, range(3))
    snaps = (0, n // 2, n)
    monkeypatch.setenv("SMO_KD_GRAPH", "0")
    dom = kdyn.KDynDomain(N)
    off = _solve(dom, RMS, members, n, cost, snaps)
    assert dom.context(RMS, DT, n, cost).get(2) == 0
    dom.drop_contexts()
    monkeypatch.delenv("SMO_KD_GRAPH")
    dom = kdyn.KDynDomain(N)
    on = _solve(dom, RMS, members, n, cost, snaps)
    assert dom.context(RMS, DT, n, cost).get(2) > 0
    dom.drop_contexts()
    for a, b in zip(off, on):
        _equal(a, b)


def test_runtime_length_kernels_at_a_tuned_size(monkeypatch):
    monkeypatch.setenv("SMO_KD_ANY", "1")
    N, n, cost = 16, 3, "Final"
    members = _members(24, range(3))
    snaps = (0, n)
    got = _batched(N, RMS, members, n, cost, snaps)
    for b, ref in enumerate(_singles(N, RMS, members, n, cost, snaps)):
        _equal(got[b], ref)


def test_permuting_the_pairs_permutes_outputs():
    N, n, cost = 16, 3, "Integrated"
    members = _members(24, range(3))
    perm = [2, 0, 1]
    a = _batched(N, RMS, members, n, cost, (n,))
    b = _batched(N, [RMS[p] for p in perm], [members[p] for p in perm], n, cost, (n,))
    for i, p in enumerate(perm):
        _equal(b[i], a[p])


def test_a_second_forward_sees_its_own_inputs_and_the_same_table():
    N, n, cost = 24, 3, "Final"                                   # G = 36: captured graphs hold the table's address
    m1, m2 = _members(36, range(3)), _members(36, range(3, 6))
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(RMS, DT, n, cost)
    J1 = ctx.forward(_stack(m1))
    J2 = ctx.forward(_stack(m2))
    g2 = ctx.adjoint(None)
    J1b = ctx.forward(_stack(m1))
    assert ctx.get(2) > 0
    dom.drop_contexts()
    assert not np.array_equal(J1, J2) and np.array_equal(J1, J1b)
    ref = _singles(N, RMS, m2, n, cost, (n,))
    L = 3 * 36 ** 3
    for b in range(3):
        assert J2[b] == ref[b][0]
        assert np.array_equal(g2[0][b * L:(b + 1) * L], ref[b][1]["Discrete"][0])
        assert np.array_equal(g2[1][b * L:(b + 1) * L], ref[b][1]["Discrete"][1])


def test_device_resident_vectors_match_the_host_path():
    N, n, cost, B = 16, 3, "Integrated", 3
    X = _stack(_members(24, range(B)))
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(RMS, DT, n, cost)
    J = ctx.forward(X)
    gh = ctx.adjoint(None, "Continuous")
    iph = ctx.inner(X[0], gh[1])
    Xd = to_device(X)
    gd = [DeviceVector(B * ctx.vec_len), DeviceVector(B * ctx.vec_len)]
    Jd = ctx.forward_dev(Xd)
    ctx.adjoint_dev(Xd, gd, "Continuous")
    ipd = ctx.inner_dev(Xd[0], gd[1])
    dom.drop_contexts()
    assert len(set(J)) == B
    assert np.array_equal(J, Jd) and np.array_equal(iph, ipd)
    assert np.array_equal(gh[0], gd[0].numpy()) and np.array_equal(gh[1], gd[1].numpy())


def _create_members(cfg, params):
    L, h = _capi.lib(), C.c_void_p()
    arr = None if params is None else (C.c_double * len(params))(*params)
    rc = L.smo_create_members(C.byref(cfg), arr, C.byref(h))
    msg = L.smo_last_error().decode()
    if h.value:
        L.smo_destroy(h)
    return rc, msg, bool(h.value)


def _cfg(kind=_capi.SMO_KDYN, batch=3, world=1, npts=16, interval=(0., 2 * np.pi), npts2=0):
    return _capi.smo_config(kind, npts, interval[0], interval[1], 1e-2, 2, 123., 0, batch, 0, 0, world, 1, npts2, 0.05, 1., 0.25)


@pytest.mark.parametrize("params,member", [(None, None), ((0.7, float("nan"), 2.9), 1), ((0.7, 1.3, 0.), 2), ((-0.7, 1.3, 2.9), 0),
                                           ((0.7, float("inf"), 2.9), 1)])
def test_argument_errors_name_the_member(params, member):
    rc, msg, made = _create_members(_cfg(), params)
    assert rc == 1 and msg and not made, (rc, msg)
    if member is not None:
        assert "member %d" % member in msg, msg


@pytest.mark.parametrize("batch", [1, 2])
def test_slabs_are_refused_also_for_one_member(batch):
    rc, msg, made = _create_members(_cfg(batch=batch, world=2), (0.7, 1.3)[:batch])
    assert rc == 1 and msg and not made, (rc, msg)
    assert "member" in msg and "world" in msg, msg


def test_kinds_with_a_tau_operator_are_refused():
    for cfg in (_cfg(_capi.SMO_SHB23, npts=64, interval=(-20., 20.)), _cfg(_capi.SMO_POIS, npts=24, interval=(0., 4 * np.pi), npts2=24)):
        rc, msg, made = _create_members(cfg, (0.7, 1.3, 2.9))
        assert rc == 6 and "tau operator" in msg and not made, (rc, msg)


def test_geometry_and_batched_refusals_are_those_of_the_uniform_batch():
    args = (_capi.SMO_KDYN, 16, (0., 2 * np.pi), 1e-2, 4)
    cm = _capi.Context(*args, RMS, cost="Integrated")
    cu = _capi.Context(*args, 1.3, cost="Integrated", batch=3)
    assert cm.params == RMS and cu.params is None and cm.batch == 3
    assert (cm.stack_bytes, cm.vec_len, cm.snapshot_len) == (cu.stack_bytes, cu.vec_len, cu.snapshot_len)
    with pytest.raises(_capi.SmoError) as e:
        cm.transform(0, np.zeros(cm.vec_len))
    assert e.value.code == 6
    assert _capi.lib().smo_kdyn_op(cm._h, 0, 0, 0, None, None, None) == 6
    cm.close(); cu.close()
