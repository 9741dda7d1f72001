"""SH23 members with their own bifurcation parameter a (smo_create_members through _capi.Context; SH23Domain fixes a): member b must equal,
bit for bit, a batch-1 context of a_b on member b's input, on the tuned (Npts = 64) and the any-length (Npts = 54) kernels, and agree with
the oracle of a_b.  (tests/test_member_params_cpu.py shows on the oracle that these values move J by > 1e-2 relative.)"""
import ctypes as C
import itertools

import numpy as np
import pytest

import parameter_cases as pc
from spheremanopt_amd import _capi

pytestmark = pytest.mark.gpu
A = (0.2, -1.7, -0.3)
INTERVAL, DT, N = pc.SH23_DEFAULT[0], 0.1, 20
ADJS = ("Discrete", "Continuous")
SNAPS = (0, 10, 20)


def _solve(Npts, a, inputs, batch=None):
    """One context (a a float: smo_create with `batch` members, a sequence: the members context); per member (J, {adj: g}, <x, g>, snapshots)."""
    ctx = _capi.Context(_capi.SMO_SH23, Npts, INTERVAL, DT, N, a, batch=len(inputs) if batch is None else batch)
    B, L = ctx.batch, ctx.vec_len
    assert B == len(inputs)
    X = np.concatenate(inputs)
    J = np.atleast_1d(ctx.forward([X]))
    g = {adj: ctx.adjoint(None, adj)[0] for adj in ADJS}
    ip = np.atleast_1d(ctx.inner(X, g[ADJS[-1]]))
    res = [(J[b], {adj: g[adj][b * L:(b + 1) * L] for adj in ADJS}, ip[b], [ctx.snapshot(i, b) for i in SNAPS]) for b in range(B)]
    ctx.close()
    return res


def _equal(x, y):
    assert x[0] == y[0] and x[2] == y[2], (x[0], y[0], x[2], y[2])
    for adj in ADJS:
        assert np.array_equal(x[1][adj], y[1][adj]), adj
    for s, t in zip(x[3], y[3]):
        assert np.array_equal(s, t)


def _inputs(Npts, same):
    return [pc.sh23_input(Npts, 42 if same else 42 + b) for b in range(3)]


@pytest.mark.parametrize("Npts", pc.SH23_NPTS)
@pytest.mark.parametrize("same_input", [True, False])
def test_members_equal_batch_one_contexts_of_their_own_a(Npts, same_input):
    inputs = _inputs(Npts, same_input)
    got = _solve(Npts, A, inputs)
    for b in range(3):
        _equal(got[b], _solve(Npts, A[b], [inputs[b]])[0])
    for x, y in itertools.combinations([r[0] for r in got], 2):
        assert x != y


@pytest.mark.parametrize("Npts", pc.SH23_NPTS)
def test_uniform_table_equals_the_shared_parameter_batch(Npts):
    inputs = _inputs(Npts, False)
    for x, y in zip(_solve(Npts, [-1.7] * 3, inputs), _solve(Npts, -1.7, inputs)):
        _equal(x, y)
    _equal(_solve(Npts, [0.2], inputs[:1])[0], _solve(Npts, 0.2, inputs[:1])[0])


@pytest.mark.parametrize("Npts", pc.SH23_NPTS)
def test_every_member_against_the_oracle_of_its_a(Npts):
    from oracle.sh23 import SH23Oracle
    inputs = _inputs(Npts, False)
    got = _solve(Npts, A, inputs)
    for b, (a, X) in enumerate(zip(A, inputs)):
        o = SH23Oracle(Npts, interval=INTERVAL, dt=DT, N_ITERS=N, a=a)
        Jo = o.forward([X])
        assert abs(got[b][0] - Jo) <= 1e-6 * abs(Jo), (b, got[b][0], Jo)
        for adj in ADJS:
            go = o.adjoint([X], adj)[0]
            d = float(np.linalg.norm(got[b][1][adj] - go) / np.linalg.norm(go))
            print("Npts %d member %d a %.1f %s: J %.3e grad %.3e" % (Npts, b, a, adj, abs(got[b][0] - Jo) / abs(Jo), d))
            assert d < 1e-6, (b, adj, d)


@pytest.mark.parametrize("params", [None, (0.2, float("nan"), -0.3)])
def test_argument_errors(params):
    L, h = _capi.lib(), C.c_void_p()
    cfg = _capi.smo_config(_capi.SMO_SH23, 64, INTERVAL[0], INTERVAL[1], DT, N, -0.3, 0, 3, 0, 0, 1, 1, 0, 0., 0., 0.)
    arr = None if params is None else (C.c_double * 3)(*params)
    assert L.smo_create_members(C.byref(cfg), arr, C.byref(h)) == 1 and not h.value
    msg = L.smo_last_error().decode()
    assert msg and (params is None or "member 1" in msg), msg
