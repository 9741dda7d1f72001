"""Windowed checkpointing of the Poiseuille snapshot stack (smo_config.ckpt = k on a SMO_POIS context): the forward solve keeps
the states 0, k, 2k, ... and N, the adjoint sweep recomputes one window of k - 1 states at a time.  Everything a ckpt = k context returns
— J, the gradient, <X, g>, every snapshot — must equal the keep-all (ckpt = 1) context's result bit for bit: Discrete and Continuous
formulation, batches, host and device vectors, dense apply, x phases as products, any call sequence, and the interval ckpt = 0 chooses.

The inputs are the oracle's synthetic_ic at DIFFERENT amplitudes (see test_poiseuille_batch_gpu.py): every batched test first asserts that
the keep-all results of its members differ."""
import numpy as np
import pytest

from spheremanopt_amd import _capi, poiseuille as pz
from spheremanopt_amd.devvec import DeviceVector, to_device

pytestmark = pytest.mark.gpu
RE, RI, DT, PR, DELTA = 500., 0.05, 5e-3, 1., 0.3
AMPS = (1., 3., 0., 0.3, 2.)                       # member b = AMPS[b] * synthetic_ic(seed 11 + b); member 2 is all zero
_ICS, _KEEPALL = {}, {}


def _members(Nx, Nz, B, continuous=False):
    from oracle.poiseuille import PoiseuilleCntsOracle, PoiseuilleOracle, synthetic_ic, synthetic_ic_cnts
    key = (Nx, Nz, continuous)
    if key not in _ICS:
        if continuous:
            o = PoiseuilleCntsOracle(Nx, Nz, Re=RE, Ri=RI, dt=DT, N_ITERS=1, s=0, Prandtl=PR, delta=DELTA)
            _ICS[key] = [synthetic_ic_cnts(o, 11 + b) for b in range(2)]
        else:
            o = PoiseuilleOracle(Nx, Nz, Re=RE, Ri=RI, dt=DT, N_ITERS=1, s=0, Prandtl=PR, delta=DELTA)
            _ICS[key] = [synthetic_ic(o, 11 + b) for b in range(len(AMPS))]
    return [AMPS[b] * _ICS[key][b] for b in range(B)]


def slots(N, k):
    """the slot count include/smo.h documents: checkpoints 0, k, ..., state N when it is no checkpoint, the window slots"""
    return N + 1 if k == 1 else N // k + 1 + (1 if N % k else 0) + min(k - 1, N - 1)


def record_bytes(Nx, Nz, k, continuous=False):
    a = (Nx - 1) // 2 + 1
    return 8 * (3 * 2 * a * Nz + (0 if k == 1 else 2 * a * 3))


def _solve(Nx, Nz, N, s, k, members, batch=1, continuous=False, dev=False):
    """forward, adjoint, inner and EVERY snapshot of `members` on one context of `batch` members and interval k (batch 1: one member after
    the other): a list of (J, gradient, <X, g>, [snapshot 0..N]) per member"""
    adj = "Continuous" if continuous else "Discrete"
    dom = pz.PoiseuilleDomain(Nx, Nz, continuous=continuous, ckpt=k)
    ctx = dom.context(RE, RI, N, DT, s, PR, DELTA, batch=batch)
    assert ctx.get(0) == min(k, N)
    L, out = ctx.vec_len, []
    for X in ([np.concatenate(members)] if batch > 1 else members):
        if dev:
            Xd, gd = to_device([X]), [DeviceVector(batch * L)]
            J = np.atleast_1d(ctx.forward_dev(Xd))
            ctx.adjoint_dev(Xd, gd, adj)
            ip = np.atleast_1d(ctx.inner_dev(Xd[0], gd[0]))
            g = gd[0].numpy()
        else:
            J = np.atleast_1d(ctx.forward([X]))
            g = ctx.adjoint(None, adj)[0]
            ip = np.atleast_1d(ctx.inner(X, g))
        for b in range(batch):
            out.append((J[b], g[b * L:(b + 1) * L].copy(), ip[b], [ctx.snapshot(i, b) for i in range(N + 1)]))
    dom.drop_contexts()
    return out


def _keepall(Nx, Nz, N, s, B=1, continuous=False, mode=""):
    """batch-1 keep-all results of the first B members, computed once per (size, steps, s, formulation, environment) and shared"""
    key = (Nx, Nz, N, s, continuous, mode)
    if key not in _KEEPALL or len(_KEEPALL[key]) < B:
        _KEEPALL[key] = _solve(Nx, Nz, N, s, 1, _members(Nx, Nz, B, continuous), continuous=continuous)
    res = _KEEPALL[key][:B]
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
    for i, (x, y) in enumerate(zip(a[3], b[3])):
        assert np.array_equal(x, y), "snapshot %d" % i


# ---- 1. the interval is honoured (both assertions fail on a library that ignores smo_config.ckpt for SMO_POIS) ---------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_interval_and_stack_bytes(B):
    Nx, Nz, N, k = 24, 24, 7, 3
    d1, d3 = pz.PoiseuilleDomain(Nx, Nz), pz.PoiseuilleDomain(Nx, Nz, ckpt=k)
    c1 = d1.context(RE, RI, N, DT, 0, PR, DELTA, batch=B)
    c3 = d3.context(RE, RI, N, DT, 0, PR, DELTA, batch=B)
    assert c1.get(0) == 1 and c3.get(0) == 3
    assert slots(N, k) == 6 and slots(N, k) <= N // k + k + 1
    assert c1.stack_bytes == (N + 1) * B * record_bytes(Nx, Nz, 1)
    assert c3.stack_bytes == slots(N, k) * B * record_bytes(Nx, Nz, k)
    assert c3.stack_bytes < c1.stack_bytes
    d1.drop_contexts(); d3.drop_contexts()


# ---- 2. Discrete, batch 1: the keep-all bits ---------------------------------------------------------------------------------------------
# 24 x 24, N = 7: k = 2, 3, 4 leave a shorter last window (3 and 4 do not divide 7 - 1 either), k = 7 = N and k = 9 > N are one window;
# 30 x 66: ragged tiles; 42 x 27: no x FFT, odd Nz; 96 x 48: several HODLR tasks per wavenumber, ada < a
CASES = [(24, 24, 7, 2), (24, 24, 7, 3), (24, 24, 7, 4), (24, 24, 7, 7), (24, 24, 7, 9), (30, 66, 5, 2), (42, 27, 5, 3), (96, 48, 4, 2)]


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("Nx,Nz,N,k", CASES)
def test_discrete_equals_keep_all(Nx, Nz, N, k, s):
    ref = _keepall(Nx, Nz, N, s)
    got = _solve(Nx, Nz, N, s, k, _members(Nx, Nz, 1))
    _equal(got[0], ref[0])


def test_device_vectors():
    ref = _keepall(24, 24, 7, 1)
    _equal(_solve(24, 24, 7, 1, 3, _members(24, 24, 1), dev=True)[0], ref[0])


@pytest.mark.parametrize("name,value", [("SMO_POIS_APPLY", "dense"), ("SMO_POIS_XFFT", "0")])
def test_dense_apply_and_x_products(name, value, monkeypatch):
    monkeypatch.setenv(name, value)
    ref = _keepall(24, 24, 7, 1, mode=name)
    _equal(_solve(24, 24, 7, 1, 3, _members(24, 24, 1))[0], ref[0])


# ---- 3. Continuous formulation (N + 1 steps, the adjoint reads the snapshots N..1 as true states) --------------------------------------
@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("Nx,Nz,N,k", [(16, 16, 6, 2), (16, 16, 6, 4), (32, 24, 7, 3)])
def test_continuous_equals_keep_all(Nx, Nz, N, k, s):
    ref = _keepall(Nx, Nz, N, s, continuous=True)
    got = _solve(Nx, Nz, N, s, k, _members(Nx, Nz, 1, True), continuous=True)
    _equal(got[0], ref[0])


# ---- 4. batches: one schedule for all members, every member the batch-1 keep-all bits -------------------------------------------------
@pytest.mark.parametrize("s", [0, 1])
def test_batch_members_equal_batch_one_keep_all(s):
    Nx, Nz, N, k, B = 24, 24, 7, 3, 3
    ref = _keepall(Nx, Nz, N, s, B)
    members = _members(Nx, Nz, B)
    got = _solve(Nx, Nz, N, s, k, members, batch=B)
    for b in range(B):
        _equal(got[b], ref[b])
    perm = [2, 0, 1]
    per = _solve(Nx, Nz, N, s, k, [members[p] for p in perm], batch=B)
    for i, p in enumerate(perm):
        _equal(per[i], got[p])


@pytest.mark.parametrize("MB", [1, 2, 4])
@pytest.mark.parametrize("s", [0, 1])
def test_batch_members_per_workgroup(s, MB, monkeypatch):
    Nx, Nz, N, k, B = 30, 66, 5, 2, 5
    ref = _keepall(Nx, Nz, N, s, B)
    monkeypatch.setenv("SMO_POIS_APPLY_MB", str(MB))
    got = _solve(Nx, Nz, N, s, k, _members(Nx, Nz, B), batch=B)
    for b in range(B):
        _equal(got[b], ref[b])


# ---- 5. call sequences: the checkpoints survive adjoints and snapshot reads, a second forward replaces them ------------------------------
@pytest.mark.parametrize("s", [0, 1])
def test_call_sequence(s):
    Nx, Nz, N, k = 24, 24, 7, 3
    ref = _keepall(Nx, Nz, N, s, 2)
    X = _members(Nx, Nz, 2)
    dom = pz.PoiseuilleDomain(Nx, Nz, ckpt=k)
    ctx = dom.context(RE, RI, N, DT, s, PR, DELTA)
    assert ctx.forward([X[0]]) == ref[0][0]
    assert np.array_equal(ctx.adjoint(None)[0], ref[0][1])
    assert np.array_equal(ctx.adjoint(None)[0], ref[0][1])
    assert np.array_equal(ctx.snapshot(5), ref[0][3][5])             # 5 is in the window of checkpoint 3; the adjoint left window 0 behind
    assert np.array_equal(ctx.adjoint(None)[0], ref[0][1])
    assert np.array_equal(ctx.snapshot(N), ref[0][3][N]) and np.array_equal(ctx.snapshot(1), ref[0][3][1])
    assert ctx.forward([X[1]]) == ref[1][0]
    assert np.array_equal(ctx.adjoint(None)[0], ref[1][1])
    dom.drop_contexts()


# ---- 6. against the oracle, once per formulation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("continuous", [False, True])
def test_against_the_oracle(continuous):
    from oracle.poiseuille import PoiseuilleCntsOracle, PoiseuilleOracle
    Nx, Nz, N, s, RTOL = (16, 16, 6, 0, 1e-6) if continuous else (24, 24, 7, 1, 1e-6)
    X = _members(Nx, Nz, 1, continuous)[0]
    o = (PoiseuilleCntsOracle if continuous else PoiseuilleOracle)(Nx, Nz, Re=RE, Ri=RI, dt=DT, N_ITERS=N, s=s, Prandtl=PR, delta=DELTA)
    Jo = o.forward([X])
    go = o.adjoint([X])[0]
    J, g, _, _ = _solve(Nx, Nz, N, s, 2, [X], continuous=continuous)[0]
    assert abs(J - Jo) <= RTOL * abs(Jo), (J, Jo)
    assert np.linalg.norm(g - go) < RTOL * np.linalg.norm(go)


# ---- 7. ckpt = 0: the smallest interval that fits, under the byte budget the chooser may assume free ------------------------------------
def test_automatic_interval(monkeypatch):
    Nx, Nz, N, s = 24, 24, 7, 1
    ref = _keepall(Nx, Nz, N, s)
    X = _members(Nx, Nz, 1)

    def create(k):
        dom = pz.PoiseuilleDomain(Nx, Nz, ckpt=k)
        return dom, dom.context(RE, RI, N, DT, s, PR, DELTA)

    monkeypatch.delenv("SMO_POIS_CKPT_BUDGET", raising=False)
    dom, ctx = create(0)
    assert ctx.get(0) == 1
    dom.drop_contexts()
    sizes = {}
    for k in range(1, N + 1):
        dom, ctx = create(k)
        sizes[k] = ctx.stack_bytes
        dom.drop_contexts()
    assert sizes[2] < sizes[1]
    monkeypatch.setenv("SMO_POIS_CKPT_BUDGET", str((sizes[1] + sizes[2]) // 2))
    dom, ctx = create(0)
    assert ctx.get(0) == 2 and ctx.stack_bytes == sizes[2]
    assert ctx.forward([X[0]]) == ref[0][0]
    assert np.array_equal(ctx.adjoint(None)[0], ref[0][1])
    for i in range(N + 1):
        assert np.array_equal(ctx.snapshot(i), ref[0][3][i])
    dom.drop_contexts()
    monkeypatch.setenv("SMO_POIS_CKPT_BUDGET", str(min(sizes.values()) - 1))
    dom = pz.PoiseuilleDomain(Nx, Nz, ckpt=0)
    with pytest.raises(_capi.SmoError) as e:
        dom.context(RE, RI, N, DT, s, PR, DELTA)
    assert e.value.code == 5                                         # SMO_ERR_NOMEM
    assert dom._ctx == {}


# ---- 8. errors, and the reference-signature callables on a ckpt domain -----------------------------------------------------------------
def test_errors(monkeypatch):
    dom = pz.PoiseuilleDomain(24, 24, ckpt=-1)
    with pytest.raises(_capi.SmoError) as e:
        dom.context(RE, RI, 4, DT, 0, PR, DELTA)
    assert e.value.code == 1                                         # SMO_ERR_ARG
    monkeypatch.setenv("SMO_POIS_XPROD", "1")
    dom2 = pz.PoiseuilleDomain(24, 24, ckpt=2)
    with pytest.raises(_capi.SmoError, match="XPROD") as e:
        dom2.context(RE, RI, 4, DT, 0, PR, DELTA)
    assert e.value.code == 6                                         # SMO_ERR_UNSUPPORTED
    assert dom._ctx == {} and dom2._ctx == {}


@pytest.mark.parametrize("s", [0, 1])
def test_reference_signature_callables(s):
    Nx, Nz, N = 24, 24, 7
    ref = _keepall(Nx, Nz, N, s)[0]
    X = _members(Nx, Nz, 1)[0]
    dom = pz.PoiseuilleDomain(Nx, Nz, ckpt=2)
    buf = pz.GEN_BUFFER(Nx, Nz, dom, N)
    args = [dom, RE, RI, N, buf, DT, s, PR, DELTA]
    assert pz.FWD_Solve_Discrete([X], *args) == ref[0]
    g = pz.ADJ_Solve_Discrete([X], *args)[0]
    assert np.array_equal(g, ref[1])
    assert pz.Inner_Prod_Discrete(X, g, dom) == ref[2]
    a = dom.a
    for i in (0, 3, N):
        want = ref[3][i].view(np.complex128).reshape(3, a, Nz)
        assert np.array_equal(buf['b_fwd'][:, :, i], want[2]) and np.array_equal(buf['u_fwd'][:, :, i], want[0])
    dom.drop_contexts()


# ---- 9. the timing classes count the replayed forward launches ---------------------------------------------------------------------------
def test_replayed_launches_are_counted_in_their_classes():
    """N = 7, k = 3: the forward solve leaves the window of 4, 5 behind, so the first adjoint replays the steps 0, 1 (states 1, 2) and a second
    one the steps 3, 4 and 0, 1: two, then four more launches of the forward operator apply, one per step."""
    Nx, Nz, N = 24, 24, 7
    X = _members(Nx, Nz, 1)[0]
    counts = {}
    for k in (1, 3):
        dom = pz.PoiseuilleDomain(Nx, Nz, ckpt=k)
        ctx = dom.context(RE, RI, N, DT, 0, PR, DELTA)
        ctx.timing_enable(True)
        ctx.forward([X]); ctx.adjoint(None)
        first = {r["kernel"]: r["launches"] for r in ctx.timing()}
        ctx.adjoint(None)
        counts[k] = (first, {r["kernel"]: r["launches"] for r in ctx.timing()})
        ctx.timing_enable(False)
        dom.drop_contexts()
    fwd = [name for name in counts[1][0] if name.startswith("pois_apply") and "transposed" not in name]
    assert len(fwd) == 1
    assert counts[1][0][fwd[0]] == N and counts[1][1][fwd[0]] == N
    assert counts[3][0][fwd[0]] == N + 2 and counts[3][1][fwd[0]] == N + 2 + 4
    adj = [name for name in counts[1][0] if "transposed" in name]
    assert counts[3][0][adj[0]] == counts[1][0][adj[0]] == N
