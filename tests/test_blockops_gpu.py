"""Gram matrix and recombination across the members of a batched context (smo_gram*, smo_combine*; csrc/blockops.hip) on the GPU.

The shapes aim at the places where the kernels can go wrong: member counts that are no multiple of the 16-row MFMA tile (1, 2, 3, 17, 33) and
one that is (16); vector lengths that are odd (G = 9, 15: every second member is only 8-byte aligned), no multiple of the chunk, smaller than
one chunk (SH23 with n = 8) and longer than one chunk per workgroup (G = 36).  Data on which ANY correct summation order gives the same bits
(small integers, needles) is compared with array_equal; random data against NumPy float64 within the worst-case bound of the two sums.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from spheremanopt_amd import _capi, kdyn, poiseuille as pz, sh23, shb23
from spheremanopt_amd.devvec import DeviceVector

pytestmark = pytest.mark.gpu

_KD = [(N, B) for N in (6, 8, 10) for B in (1, 2, 3, 16, 17, 33)] + [(24, 3), (24, 17)]
_SH = [(N, B) for N in (4, 6, 256) for B in (1, 5, 17, 64)]
CASES = [("kdyn",) + c for c in _KD] + [("sh23",) + c for c in _SH]
_IDS = ["%s-N%d-B%d" % c for c in CASES]
U52 = 2. ** -52


@functools.lru_cache(maxsize=None)
def _context(kind, N, B):
    """One context per case for the whole module (one step: only the vector geometry matters); scale = the divisor of its inner product."""
    if kind == "kdyn":
        dom = kdyn.KDynDomain(N)
        return dom.context(1., 1e-3, 1, "Final", batch=B), np.float64(dom.G ** 3)
    dom = sh23.SH23Domain(N)
    return dom.context(0.1, 1, batch=B), np.float64(dom.G)


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for kind, N, B in CASES:
        if (kind, N, B) in _opened:
            _context(kind, N, B)[0].close()
    _context.cache_clear()


_opened = set()


def _case(kind, N, B):
    _opened.add((kind, N, B))
    ctx, scale = _context(kind, N, B)
    assert ctx.batch == B
    return ctx, scale, ctx.vec_len


@functools.lru_cache(maxsize=None)
def _integer_data(n, B):
    """x, y with entries in [-8, 8] and their exact Gram matrix (computed once per shape, shared, read-only)."""
    rs = np.random.RandomState(1000 * B + n % 997)
    x, y = (rs.randint(-8, 9, (B, n)).astype(np.float64) for _ in range(2))
    xi, yi = x.astype(np.int64), y.astype(np.int64)
    for a in (x, y):
        a.setflags(write=False)
    return x, y, xi @ yi.T, xi @ xi.T


def _permutations(B, rs):
    """Identity, rotation by one, reversal, a swap across every 16-row tile boundary the batch has, and one seeded random permutation."""
    ident = np.arange(B)
    perms = [ident, np.roll(ident, 1), ident[::-1].copy()]
    for edge in range(16, B, 16):
        p = ident.copy()
        p[[edge - 1, edge]] = p[[edge, edge - 1]]
        perms.append(p)
    perms.append(rs.permutation(B))
    return perms


def _dev(a):
    return DeviceVector.from_numpy(np.ascontiguousarray(a).reshape(-1))


# ---- 1. exact on integers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,B", CASES, ids=_IDS)
def test_gram_and_combine_are_exact_on_integers(kind, N, B):
    ctx, scale, n = _case(kind, N, B)
    x, y, Gxy, Gxx = _integer_data(n, B)
    X, Y = _dev(x), _dev(y)
    want = Gxy.astype(np.float64) / scale
    assert np.array_equal(ctx.gram(x, y), want)
    assert np.array_equal(ctx.gram_dev(X, Y), want)
    rs = np.random.RandomState(B)
    for perm in _permutations(B, rs):                                    # the members of y permuted: the columns of the Gram matrix permuted
        assert np.array_equal(ctx.gram_dev(X, _dev(y[perm])), want[:, perm]), perm
    S = ctx.gram_dev(X)
    assert np.array_equal(S, Gxx.astype(np.float64) / scale)
    assert np.array_equal(S, S.T) and np.array_equal(ctx.gram(x), S)
    assert np.array_equal(ctx.gram_dev(X, X), S)
    Cm = rs.randint(-4, 5, (B, B)).astype(np.float64)
    want_c = (Cm.astype(np.int64).T @ x.astype(np.int64)).astype(np.float64)
    assert np.array_equal(ctx.combine(Cm, x).reshape(B, n), want_c)
    assert np.array_equal(ctx.combine_dev(Cm, X).numpy().reshape(B, n), want_c)


# ---- 2. needles ---------------------------------------------------------------------------------------------------------------------------
def _needles(ctx, n):
    """First, second-to-last and last element, and both sides of the seams the kernels have: the first and last chunk boundary, the first and
    last workgroup boundary of block_gram, the first and last workgroup boundary of block_combine."""
    g = ctx.gram_geometry()
    kc, wg, cw = g["chunk"], g["chunk"] * g["chunks_per_workgroup"], g["combine_workgroup"]
    idx = {0, n - 2, n - 1}
    for step in (kc, wg, cw):
        for m in {step, ((n - 1) // step) * step}:
            idx.update((m - 1, m))
    return sorted(i for i in idx if 0 <= i < n), kc


@pytest.mark.parametrize("kind,N,B", CASES, ids=_IDS)
def test_needles(kind, N, B):
    """x_a = e_i, y_b = 1: exactly 1 / scale in row a and 0 elsewhere — at the ends, at the first and last seam of every kind, at the sizes up to
    G = 15 on both sides of EVERY chunk boundary one needle at a time; and at every size x_a = 1 on both sides of all of them at once: the count / scale."""
    ctx, scale, n = _case(kind, N, B)
    idx, kc = _needles(ctx, n)
    Y = _dev(np.ones((B, n)))
    x = np.zeros((B, n))
    for j, i in enumerate(idx):
        a = j % B
        x[a, i] = 1.
        want = np.zeros((B, B))
        want[a, :] = 1. / scale
        got = ctx.gram_dev(_dev(x), Y)
        assert np.array_equal(got, want), (i, a, got)
        # the recombination moves the needle of member a to member (a + 1) % B, same element, nothing else
        Cm = np.zeros((B, B))
        Cm[a, (a + 1) % B] = 3.
        out = ctx.combine_dev(Cm, _dev(x)).numpy().reshape(B, n)
        assert out[(a + 1) % B, i] == 3. and np.count_nonzero(out) == 1, (i, a)
        x[a, i] = 0.
    if n <= 10125:                                                       # the small sizes: a needle of its own on both sides of EVERY chunk boundary
        for j, i in enumerate(i for m in range(kc, n, kc) for i in (m - 1, m)):
            a = j % B
            x[a, i] = 1.
            want = np.zeros((B, B))
            want[a, :] = 1. / scale
            assert np.array_equal(ctx.gram_dev(_dev(x), Y), want), (i, a)
            x[a, i] = 0.
    a = B - 1
    seams = np.arange(kc, n, kc)
    hot = np.unique(np.concatenate([seams - 1, seams])) if seams.size else np.array([0])
    x[a, hot] = 1.
    want = np.zeros((B, B))
    want[a, :] = np.float64(hot.size) / scale
    assert np.array_equal(ctx.gram_dev(_dev(x), Y), want)


# ---- 3. guards ----------------------------------------------------------------------------------------------------------------------------
def _guarded(a, fill=np.nan):
    """The data with 3 doubles of NaN before and 5 after, on the device; the view starts at an odd element: 8-byte aligned only."""
    buf = np.full(a.size + 8, fill)
    buf[3:3 + a.size] = np.asarray(a).reshape(-1)
    return DeviceVector.from_numpy(buf)


@pytest.mark.parametrize("kind,N,B", CASES, ids=_IDS)
def test_views_with_nan_guards(kind, N, B):
    ctx, scale, n = _case(kind, N, B)
    x, y, Gxy, _ = _integer_data(n, B)
    L = _capi.lib()
    gx, gy = _guarded(x), _guarded(y)
    assert (gx.ptr + 24) % 16 == 8
    out = np.full((B, B), np.nan)
    _capi._check(L.smo_gram_dev(ctx._h, C.c_void_p(gx.ptr + 24), C.c_void_p(gy.ptr + 24), out.ctypes.data_as(_capi._dp)))
    assert np.all(np.isfinite(out))
    assert np.array_equal(out, ctx.gram_dev(_dev(x), _dev(y))) and np.array_equal(out, Gxy.astype(np.float64) / scale)
    sym = np.full((B, B), np.nan)
    _capi._check(L.smo_gram_dev(ctx._h, C.c_void_p(gx.ptr + 24), C.c_void_p(gx.ptr + 24), sym.ctypes.data_as(_capi._dp)))
    assert np.array_equal(sym, ctx.gram_dev(_dev(x)))
    Cm = np.random.RandomState(B).randint(-4, 5, (B, B)).astype(np.float64)
    go = _guarded(np.zeros(B * n))
    _capi._check(L.smo_combine_dev(ctx._h, Cm.ctypes.data_as(_capi._dp), C.c_void_p(gx.ptr + 24), C.c_void_p(go.ptr + 24)))
    res = go.numpy()
    assert np.all(np.isnan(res[:3])) and np.all(np.isnan(res[-5:]))          # the guards around `out` are untouched
    assert np.array_equal(res[3:-5].reshape(B, n), (Cm.astype(np.int64).T @ x.astype(np.int64)).astype(np.float64))


# ---- 4. selection and scaling -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_data(n, B):
    rs = np.random.RandomState(7 * B + n % 991)
    x = rs.standard_normal((B, n)) * 10. ** rs.randint(-3, 4, (B, n))
    y = rs.standard_normal((B, n))
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@pytest.mark.parametrize("kind,N,B", CASES, ids=_IDS)
def test_selection_and_scaling_are_exact(kind, N, B):
    ctx, scale, n = _case(kind, N, B)
    x, _ = _random_data(n, B)
    X = _dev(x)
    assert np.all(ctx.combine_dev(np.eye(B), X).numpy().reshape(B, n) == x)
    rs = np.random.RandomState(3 * B)
    perm = rs.permutation(B)
    P = np.zeros((B, B))
    P[perm, np.arange(B)] = 1.                                              # out_b = x_perm[b]
    assert np.array_equal(ctx.combine_dev(P, X).numpy().reshape(B, n), x[perm])
    s = rs.standard_normal(B) * 3.
    want = DeviceVector(B * n)
    for b in range(B):
        _capi._check(_capi.lib().smo_vec_axpby(0, n, float(s[b]), C.c_void_p(X.ptr + 8 * b * n), 0.0, None, C.c_void_p(want.ptr + 8 * b * n)))
    assert np.array_equal(ctx.combine_dev(np.diag(s), X).numpy(), want.numpy())
    assert np.array_equal(ctx.combine(np.diag(s), x), want.numpy())


# ---- 5. random data against NumPy float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,B", CASES, ids=_IDS)
def test_random_data_within_the_worst_case_bound(kind, N, B):
    """Gram: |delta| <= (n + 2) 2^-52 sum_k |x_a[k] y_b[k]| / scale (the device's sum plus NumPy's, worst case); combine:
    |delta| <= (B + 2) 2^-52 sum_a |C[a][b] x_a[k]|.  Two calls return identical bits."""
    ctx, scale, n = _case(kind, N, B)
    x, y = _random_data(n, B)
    X, Y = _dev(x), _dev(y)
    got = ctx.gram_dev(X, Y)
    bound = (n + 2) * U52 * (np.abs(x) @ np.abs(y).T) / scale
    err = np.abs(got - (x @ y.T) / scale)
    print("gram   worst |delta| / bound = %.3g" % (err / bound).max())
    assert np.all(err <= bound)
    assert np.array_equal(got, ctx.gram_dev(X, Y))
    S = ctx.gram_dev(X)
    assert np.all(np.abs(S - (x @ x.T) / scale) <= (n + 2) * U52 * (np.abs(x) @ np.abs(x).T) / scale)
    assert np.array_equal(S, S.T) and np.array_equal(S, ctx.gram_dev(X))
    Cm = np.random.RandomState(B + 11).standard_normal((B, B))
    out = ctx.combine_dev(Cm, X)
    bound = (B + 2) * U52 * (np.abs(Cm).T @ np.abs(x))
    err = np.abs(out.numpy().reshape(B, n) - Cm.T @ x)
    print("combine worst |delta| / bound = %.3g" % (err / np.maximum(bound, np.finfo(float).tiny)).max())
    assert np.all(err <= bound)
    assert np.array_equal(out.numpy(), ctx.combine_dev(Cm, X).numpy())


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
def _codes(ctx):
    """Return codes of the four entry points on valid, distinct device buffers."""
    L, n = _capi.lib(), ctx.vec_len * ctx.batch
    X, Y, O = DeviceVector(n), DeviceVector(n), DeviceVector(n)
    g = np.zeros(ctx.batch * ctx.batch)
    Cm = np.eye(ctx.batch)
    h, ho = np.zeros(n), np.zeros(n)
    return (L.smo_gram_dev(ctx._h, X.ptr, Y.ptr, g.ctypes.data_as(_capi._dp)), L.smo_gram(ctx._h, h.ctypes.data, h.ctypes.data, g.ctypes.data_as(_capi._dp)),
            L.smo_combine_dev(ctx._h, Cm.ctypes.data_as(_capi._dp), X.ptr, O.ptr), L.smo_combine(ctx._h, Cm.ctypes.data_as(_capi._dp), h.ctypes.data, ho.ctypes.data))


def test_weighted_inner_products_and_large_batches_are_refused():
    UNSUPPORTED, ARG = 6, 1
    dom = shb23.SHBDomain(64)
    ctx = dom.context(1e-2, 1, batch=2)
    assert _codes(ctx) == (UNSUPPORTED,) * 4
    assert "weights" in _capi.lib().smo_last_error().decode()
    dom.drop_contexts()
    pdom = pz.PoiseuilleDomain(24, 24)
    assert _codes(pdom.context(500., 0.05, 1, 5e-3, 0, 1., 0.3, batch=2)) == (UNSUPPORTED,) * 4
    pdom.drop_contexts()
    ctx = sh23.SH23Domain(4).context(0.1, 1, batch=257)
    assert _codes(ctx) == (UNSUPPORTED,) * 4
    assert "256" in _capi.lib().smo_last_error().decode()
    ctx.close()
    ctx, _, n = _case("kdyn", 6, 3)
    L = _capi.lib()
    big = DeviceVector(2 * 3 * n)
    Cm = np.eye(3)
    for off in (0, 8, 8 * (3 * n - 1)):                                     # out == x, shifted by one element, the last element of x
        assert L.smo_combine_dev(ctx._h, Cm.ctypes.data_as(_capi._dp), C.c_void_p(big.ptr), C.c_void_p(big.ptr + off)) == ARG
        assert L.smo_combine_dev(ctx._h, Cm.ctypes.data_as(_capi._dp), C.c_void_p(big.ptr + off), C.c_void_p(big.ptr)) == ARG
    assert L.smo_combine_dev(ctx._h, Cm.ctypes.data_as(_capi._dp), C.c_void_p(big.ptr), C.c_void_p(big.ptr + 8 * 3 * n)) == 0      # adjacent: fine
    h = np.zeros(2 * 3 * n)
    assert L.smo_combine(ctx._h, Cm.ctypes.data_as(_capi._dp), h.ctypes.data, h.ctypes.data + 8) == ARG
    g = np.zeros(9)
    assert L.smo_gram_dev(ctx._h, None, C.c_void_p(big.ptr), g.ctypes.data_as(_capi._dp)) == ARG
    assert L.smo_gram_dev(ctx._h, C.c_void_p(big.ptr + 4), C.c_void_p(big.ptr), g.ctypes.data_as(_capi._dp)) == ARG
    assert L.smo_combine_dev(ctx._h, Cm.ctypes.data_as(_capi._dp), C.c_void_p(big.ptr + 4), C.c_void_p(big.ptr + 8 * 3 * n)) == ARG
    assert L.smo_combine_dev(ctx._h, None, C.c_void_p(big.ptr), C.c_void_p(big.ptr + 8 * 3 * n)) == ARG


# ---- 7. state -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["full", "frozen", "frozen-no-states", "horizons"])
def test_gram_between_forward_and_adjoint_leaves_the_gradient_alone(mode):
    """forward_dev, gram_dev (and combine_dev), adjoint_dev: the gradient has the bits of the run without the calls in between."""
    B = 3
    dom = kdyn.KDynDomain(8)
    if mode == "full":
        ctx = dom.context(1.3, 1e-2, 4, "Final", batch=B)
    elif mode == "horizons":
        ctx = dom.context(1.3, 1e-2, (4, 2, 3), "Final")
    else:
        ctx = dom.context(1.3, 1e-2, 4, "Final", batch=B, frozen_U=True, keep_states=(mode == "frozen"))
    n = ctx.vec_len
    X = [_dev(np.concatenate([kdyn.synthetic_field(dom.G, 10 * c + b + 1) for b in range(B)])) for c in range(2)]

    def gradients(between):
        grads = [DeviceVector(B * n) for _ in range(ctx.ngrad)]
        J = np.atleast_1d(ctx.forward_dev(X)).copy()
        if between:
            G = ctx.gram_dev(X[0], X[1])
            ctx.gram_dev(X[0])
            ctx.combine_dev(np.eye(B)[::-1].copy(), X[0])
            assert np.all(np.isfinite(G))
        ctx.adjoint_dev(X, grads)
        return J, [g.numpy() for g in grads]

    J0, g0 = gradients(False)
    J1, g1 = gradients(True)
    assert np.array_equal(J0, J1)
    for a, b in zip(g0, g1):
        assert np.array_equal(a, b) and np.any(a != 0.)
    dom.drop_contexts()
