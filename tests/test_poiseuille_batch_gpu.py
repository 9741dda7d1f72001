"""Batched plane-Poiseuille solves (smo_config.batch = B > 1, Discrete formulation): B independent problems per call that share one set of
tau operators.  Member b of a batch must equal, bit for bit, a batch-1 solve of member b's input — J, the gradient, <x_b, g_b> and the
snapshots — with host vectors and device vectors, under a permutation of the members, with the dense apply, and whatever number of
members one workgroup of the HODLR apply serves (SMO_POIS_APPLY_MB).

The members are the oracle's synthetic_ic at DIFFERENT amplitudes plus an all-zero one: at s = 1 the base density dominates J and two
seeds of equal amplitude differ in its 7th digit only, so every test first asserts that the batch-1 results of its members differ."""
import numpy as np
import pytest

from spheremanopt_amd import _capi, poiseuille as pz
from spheremanopt_amd.devvec import DeviceVector, to_device

pytestmark = pytest.mark.gpu
RE, RI, DT, PR, DELTA = 500., 0.05, 5e-3, 1., 0.3
AMPS = (1., 3., 0., 0.3, 2.)                       # member b = AMPS[b] * synthetic_ic(seed 11 + b); member 2 is all zero
# Nx x Nz -> steps.  24 x 24: smallest x FFT;  30 x 66: ragged last tile of 8 z columns, GEMM tiles ragged both ways;  42 x 27: no x FFT
# instantiation and odd Nz, every x phase a GEMM;  96 x 48: HODLR split depth 3 with several tasks per wavenumber, ada < a
STEPS = {(24, 24): 4, (30, 66): 3, (42, 27): 3, (96, 48): 3}
_ICS, _SINGLES = {}, {}


def _members(Nx, Nz, B, amps=AMPS):
    from oracle.poiseuille import PoiseuilleOracle, synthetic_ic
    if (Nx, Nz) not in _ICS:
        o = PoiseuilleOracle(Nx, Nz, Re=RE, Ri=RI, dt=DT, N_ITERS=1, s=0, Prandtl=PR, delta=DELTA)
        _ICS[(Nx, Nz)] = [synthetic_ic(o, 11 + b) for b in range(len(AMPS))]
    return [amps[b] * _ICS[(Nx, Nz)][b] for b in range(B)]


def _snaps(n):
    return (0, (n + 1) // 2, n)


def _solve(Nx, Nz, s, members, batch):
    """forward, adjoint, inner and snapshots of `members` on ONE context of `batch` members (batch = 1: one member after the other)."""
    n = STEPS[(Nx, Nz)]
    dom = pz.PoiseuilleDomain(Nx, Nz)
    ctx = dom.context(RE, RI, n, DT, s, PR, DELTA, batch=batch)
    L, out = ctx.vec_len, []
    for X in ([np.concatenate(members)] if batch > 1 else members):
        J = np.atleast_1d(ctx.forward([X]))
        g = ctx.adjoint(None)[0]
        ip = np.atleast_1d(ctx.inner(X, g))
        for b in range(batch):
            out.append((J[b], g[b * L:(b + 1) * L].copy(), ip[b], [ctx.snapshot(i, b) for i in _snaps(n)]))
    dom.drop_contexts()
    return out


def _singles(Nx, Nz, s, B, mode="hodlr"):
    """batch-1 results of the first B members, computed once per (size, s, apply mode) and shared; asserted pairwise different."""
    key = (Nx, Nz, s, mode)
    if key not in _SINGLES or len(_SINGLES[key]) < B:
        _SINGLES[key] = _solve(Nx, Nz, s, _members(Nx, Nz, len(AMPS)), 1)
    res = _SINGLES[key][:B]
    for i in range(B):
        for j in range(i):
            assert res[i][0] != res[j][0] and not np.array_equal(res[i][1], res[j][1]), (i, j)
            assert not np.array_equal(res[i][3][-1], res[j][3][-1]), (i, j)
    return res


def _equal(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert np.array_equal(a[1], b[1])
    assert a[2] == b[2], (a[2], b[2])
    assert len(a[3]) == len(b[3])
    for x, y in zip(a[3], b[3]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("Nx,Nz,B", [(24, 24, 3), (30, 66, 3), (42, 27, 3), (96, 48, 2)])
def test_members_equal_batch_one_runs(Nx, Nz, B, s):
    ref = _singles(Nx, Nz, s, B)
    members = _members(Nx, Nz, B)
    got = _solve(Nx, Nz, s, members, B)
    for b in range(B):
        _equal(got[b], ref[b])
    # device-resident vectors
    n = STEPS[(Nx, Nz)]
    dom = pz.PoiseuilleDomain(Nx, Nz)
    ctx = dom.context(RE, RI, n, DT, s, PR, DELTA, batch=B)
    L = ctx.vec_len
    Xd = to_device([np.concatenate(members)])
    gd = [DeviceVector(B * L)]
    J = np.atleast_1d(ctx.forward_dev(Xd))
    ctx.adjoint_dev(Xd, gd)
    ip = np.atleast_1d(ctx.inner_dev(Xd[0], gd[0]))
    g = gd[0].numpy()
    dev = [(J[b], g[b * L:(b + 1) * L], ip[b], [ctx.snapshot(i, b) for i in _snaps(n)]) for b in range(B)]
    dom.drop_contexts()
    for b in range(B):
        _equal(dev[b], ref[b])


@pytest.mark.parametrize("Nx,Nz", [(24, 24), (30, 66)])
def test_permuting_members_permutes_outputs(Nx, Nz):
    s, perm = 1, [2, 0, 1]
    ref = _singles(Nx, Nz, s, 3)
    members = _members(Nx, Nz, 3)
    a = _solve(Nx, Nz, s, members, 3)
    b = _solve(Nx, Nz, s, [members[p] for p in perm], 3)
    for i, p in enumerate(perm):
        _equal(b[i], a[p])
        _equal(b[i], ref[p])


# B = 5: ragged last group (2 + 2 + 1, 4 + 1); B = 3 with MB = 4: a group larger than the batch.  The forward apply runs over the ada
# de-aliased modes, the transposed one (with the in-kernel q . lambda extras) over all a modes.
@pytest.mark.parametrize("B,MB", [(5, 1), (5, 2), (5, 4), (3, 4)])
@pytest.mark.parametrize("s", [1, 0])
@pytest.mark.parametrize("Nx,Nz", [(30, 66), (96, 48)])
def test_members_per_workgroup_of_the_hodlr_apply(Nx, Nz, s, B, MB, monkeypatch):
    ref = _singles(Nx, Nz, s, B)
    monkeypatch.setenv("SMO_POIS_APPLY_MB", str(MB))
    got = _solve(Nx, Nz, s, _members(Nx, Nz, B), B)
    for b in range(B):
        _equal(got[b], ref[b])


@pytest.mark.parametrize("Nx,Nz", [(24, 24), (42, 27)])
def test_dense_apply(Nx, Nz, monkeypatch):
    monkeypatch.setenv("SMO_POIS_APPLY", "dense")
    for s in (0, 1):
        ref = _singles(Nx, Nz, s, 3, mode="dense")
        got = _solve(Nx, Nz, s, _members(Nx, Nz, 3), 3)
        for b in range(3):
            _equal(got[b], ref[b])


@pytest.mark.parametrize("s", [0, 1])
def test_members_against_the_oracle(s):
    """1e-6 relative (the project's tolerance against the oracle); the members' oracle values differ from each other by more than 100 x that,
    so a swapped or repeated member cannot pass.  (s = 1: the base density dominates J, hence the large amplitudes.)"""
    from oracle.poiseuille import PoiseuilleOracle
    Nx, Nz, B, RTOL = 24, 24, 3, 1e-6
    n = STEPS[(Nx, Nz)]
    members = _members(Nx, Nz, B, amps=(1., 100., 200.))
    o = PoiseuilleOracle(Nx, Nz, Re=RE, Ri=RI, dt=DT, N_ITERS=n, s=s, Prandtl=PR, delta=DELTA)
    Jo = [o.forward([X]) for X in members]
    go = []
    for X in members:
        o.forward([X])
        go.append(o.adjoint([X])[0])
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))   # noqa: E731
    for i in range(B):
        for j in range(i):
            assert abs(Jo[i] - Jo[j]) > 100 * RTOL * max(abs(Jo[i]), abs(Jo[j])), (i, j, Jo)
            assert rel(go[i], go[j]) > 100 * RTOL
    dom = pz.PoiseuilleDomain(Nx, Nz)
    ctx = dom.context(RE, RI, n, DT, s, PR, DELTA, batch=B)
    X = np.concatenate(members)
    J = ctx.forward([X])
    g = ctx.adjoint(None)[0]
    ip = ctx.inner(X, g)
    dom.drop_contexts()
    L = 2 * Nx * Nz
    for b in range(B):
        assert abs(J[b] - Jo[b]) <= RTOL * abs(Jo[b]), (b, J[b], Jo[b])
        assert rel(g[b * L:(b + 1) * L], go[b]) < RTOL, b
        ipo = o.inner(members[b], go[b])
        assert abs(ip[b] - ipo) <= RTOL * abs(ipo), (b, ip[b], ipo)


def _apply_rows(t):
    return [r for r in t if r["kernel"].startswith("pois_apply")]


def test_stack_and_apply_bytes(monkeypatch):
    Nx, Nz, n, B = 30, 66, 3, 4
    dom = pz.PoiseuilleDomain(Nx, Nz)
    c1 = dom.context(RE, RI, n, DT, 0, PR, DELTA)
    t1 = _apply_rows(c1.timing())
    assert len(t1) == 2 and all(r["hbm_bytes_per_launch"] > 0 for r in t1)
    for MB, factor in ((1, 4), (4, 1)):                              # the operators are read once per group of MB members
        monkeypatch.setenv("SMO_POIS_APPLY_MB", str(MB))
        d = pz.PoiseuilleDomain(Nx, Nz)
        cb = d.context(RE, RI, n, DT, 0, PR, DELTA, batch=B)
        assert cb.stack_bytes == B * c1.stack_bytes and cb.vec_len == c1.vec_len and cb.snapshot_len == c1.snapshot_len
        tb = _apply_rows(cb.timing())
        assert [r["kernel"] for r in tb] == [r["kernel"] for r in t1]
        for r1, rb in zip(t1, tb):
            assert rb["bytes_per_launch"] == factor * r1["bytes_per_launch"]
            assert rb["hbm_bytes_per_launch"] == factor * r1["hbm_bytes_per_launch"]
        d.drop_contexts()
    dom.drop_contexts()


def test_errors(monkeypatch):
    Nx, Nz, n = 24, 24, 2
    dom = pz.PoiseuilleDomain(Nx, Nz)
    ctx = dom.context(RE, RI, n, DT, 0, PR, DELTA, batch=2)
    X = np.concatenate(_members(Nx, Nz, 2))
    ctx.forward([X])
    ctx.snapshot(n, 1)
    with pytest.raises(_capi.SmoError) as e:
        ctx.snapshot(n, 2)                                           # member index beyond the batch
    assert e.value.code == 1
    with pytest.raises(_capi.SmoError) as e:
        ctx.transform(0, np.zeros(Nx * Nz), out_len=2 * dom.a * Nz)
    assert e.value.code == 6                                         # SMO_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        ctx.forward([X[:ctx.vec_len]])                               # one member's vector on a batch-2 context
    dom.drop_contexts()
    for cost in (2, 3):                                              # the Continuous formulation keeps refusing a batch, and says so
        with pytest.raises(_capi.SmoError, match="Continuous") as e:
            _capi.Context(_capi.SMO_POIS, 16, (0., 4. * np.pi), DT, n, RE, cost=cost, batch=2, npts2=16, param2=RI, param3=PR, param4=DELTA)
        assert e.value.code == 1
    with pytest.raises(_capi.SmoError, match="1024") as e:           # beyond what blockIdx.z of the batched products carries
        dom.context(RE, RI, n, DT, 0, PR, DELTA, batch=1025)
    assert e.value.code == 6
    monkeypatch.setenv("SMO_POIS_APPLY_MB", "3")
    with pytest.raises(_capi.SmoError) as e:
        dom.context(RE, RI, n, DT, 0, PR, DELTA, batch=2)
    assert e.value.code == 1
    # Nz = 384 with one task per wavenumber (split depth 0): one member's Z array takes 66 KB or more, four do not fit the 160 KB of a workgroup
    monkeypatch.setenv("SMO_POIS_APPLY_MB", "4")
    monkeypatch.setenv("SMO_POIS_HODLR_SPLIT", "0")
    big = pz.PoiseuilleDomain(12, 384)
    with pytest.raises(_capi.SmoError, match="LDS") as e:
        big.context(RE, RI, 1, DT, 0, PR, DELTA, batch=2)
    assert e.value.code == 1
    assert dom._ctx == {} and big._ctx == {}
