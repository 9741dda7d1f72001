"""SH23 members with a time horizon of their own (smo_set_horizons): member b must equal, bit for bit, a batch-1 context created with
n_iters = N_b on member b's input — J, the gradient of both adjoint types, <x_b, y_b> and the snapshots —, on an instantiated length and on the
run-time-length kernels, with one `a` per member as well."""
import numpy as np
import pytest

from parameter_cases import sh23_input
from spheremanopt_amd import _capi, sh23

pytestmark = pytest.mark.gpu
DT, CAP, HZ = 0.1, 20, (20, 1, 7, 20)
BOX = (0., 12. * np.pi)
ADJS = ("Discrete", "Continuous")


def _inputs(Npts):
    return [sh23_input(Npts, seed=42 + b) for b in range(len(HZ))]


def _solve(ctx, xs, hz):
    B, G = len(xs), xs[0].size
    X = np.concatenate(xs)
    J = np.atleast_1d(ctx.forward([X]))
    g = {adj: ctx.adjoint(None, adj)[0] for adj in ADJS}
    ip = np.atleast_1d(ctx.inner(X, g["Continuous"]))
    return [(J[b], {adj: g[adj][b * G:(b + 1) * G] for adj in ADJS}, ip[b], [ctx.snapshot(i, b) for i in (0, hz[b] // 2, hz[b])]) for b in range(B)]


def _equal(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for adj in ADJS:
        assert np.array_equal(a[1][adj], b[1][adj]), adj
    assert a[2] == b[2]
    for s, t in zip(a[3], b[3]):
        assert np.array_equal(s, t)


def _single(Npts, x, nb, a=sh23.A_PARAM):
    ctx = _capi.Context(_capi.SMO_SH23, Npts, BOX, DT, nb, a)
    res = _solve(ctx, [x], [nb])[0]
    ctx.close()
    return res


# 64: an instantiated length;  66 = 2 * 3 * 11: no instantiation, the run-time-length kernels
@pytest.mark.parametrize("Npts", [64, 66])
def test_members_equal_batch_one_contexts_of_their_own_horizon(Npts):
    xs = _inputs(Npts)
    dom = sh23.SH23Domain(Npts)
    ctx = dom.context(DT, HZ)
    assert ctx.horizons == HZ and ctx.batch == 4 and ctx.cfg.n_iters == CAP
    got = _solve(ctx, xs, HZ)
    with pytest.raises(_capi.SmoError) as e:
        ctx.snapshot(2, 1)                                        # member 1 has states 0 and 1
    assert e.value.code == 1
    plain_bytes = ctx.stack_bytes
    # back to the plain batch, and to other values
    ctx.set_horizons(None)
    with pytest.raises(_capi.SmoError) as e:
        ctx.adjoint(None)
    assert e.value.code == 4
    plain = _solve(ctx, xs, (CAP,) * 4)
    ctx.set_horizons((3, CAP, 3, 5))
    other = _solve(ctx, xs, (3, CAP, 3, 5))
    dom.drop_contexts()
    ref = _capi.Context(_capi.SMO_SH23, Npts, BOX, DT, CAP, sh23.A_PARAM, batch=4)
    assert ref.stack_bytes == plain_bytes                          # the capacity
    for a, b in zip(plain, _solve(ref, xs, (CAP,) * 4)):
        _equal(a, b)
    ref.close()
    for b, nb in enumerate(HZ):
        _equal(got[b], _single(Npts, xs[b], nb))
    for b, nb in enumerate((3, CAP, 3, 5)):
        _equal(other[b], _single(Npts, xs[b], nb))
    assert len({r[0] for r in got}) == 4


def test_one_a_per_member_as_well():
    Npts, avals = 64, (-0.3, -0.1, 0.2, -0.5)
    xs = _inputs(Npts)
    ctx = _capi.Context(_capi.SMO_SH23, Npts, BOX, DT, CAP, avals)
    ctx.set_horizons(HZ)
    got = _solve(ctx, xs, HZ)
    ctx.close()
    for b, nb in enumerate(HZ):
        _equal(got[b], _single(Npts, xs[b], nb, avals[b]))


def test_bad_values_name_the_member():
    ctx = _capi.Context(_capi.SMO_SH23, 64, BOX, DT, CAP, sh23.A_PARAM, batch=2)
    for bad, k in (((5, 0), 1), ((CAP + 1, 5), 0)):
        with pytest.raises(_capi.SmoError) as e:
            ctx.set_horizons(bad)
        assert e.value.code == 1 and "member %d" % k in str(e.value)
    ctx.close()
