"""No kernel may write outside the block it was handed (SMO_GUARD: csrc/guard.hpp, guard.hip; the counterpart for writes of test_poison_gpu.py).

With SMO_GUARD=<cap> every device block of the library — each buffer of each context (DevPool::alloc) and each device vector (smo_vec_alloc)
— lies between two zones of a position-dependent pattern, each as long as the block itself (at least 4096 bytes, at most the cap: 64 MiB
here), and the slack between the requested bytes and the next multiple of 256 carries the pattern too.  Zones and slack are compared on the
device when the block is given back, and smo_guard_report adds up what was found.

(a) every case of poison_ops.CASES, and the one-item shape of the adjoint x pass at 128^3, runs with the knob unset and set: the same bits in
    order of production, the same path indicators, and after the contexts are gone and the vector pool is released damaged == 0 with
    checked >= 1.  A condition, not a tolerance; no case is skipped and no block is exempt.
(b) device vectors under the knob: the algebra equals NumPy's at sizes with 8, 0 and 248 bytes of slack and past one pass of the kernel; the
    one-element-per-lane kernel on views at an odd offset; forward_dev / adjoint_dev / hessvec_dev / combine_dev writing into DeviceVectors.
(c) the detector sees a device write: five single stores through smo_vec_axpby, each INSIDE the zones this library allocated around an
    n = 33 vector (asserted from the zone rule before each call), are each reported once, with the zone and the byte offset.  A damaged block
    is patterned again by the report, so a second report gives 0 until the next store.
(d) the knob acts at the DevPool site and changes nothing else: byte counts, path indicators, alignment; unset, the report is 0 / 0; and one
    case per family under SMO_GUARD and SMO_POISON=255 together.
(e) a value that is no cap is an argument error at both allocation sites.

On an MI355X: 147 tests in 15.6 s, none damaged; the slowest are kdyn-256-Final-Discrete (4.0 s for both runs and their checks, zones of
64 MiB around blocks of up to 1.4 GB) and shb23-1023 (2.4 s); kdyn-128 takes 0.5 s.  test_poison_gpu.py, in the same session: 143 tests in
22.8 s (kdyn-256: 8.3 s for its four runs).
"""
import ctypes as C
import gc

import numpy as np
import pytest

import poison_ops as po
import test_kdyn_adj_x_shape_gpu as x_shape
from test_poison_gpu import _first_difference
from spheremanopt_amd import _capi, devvec
from spheremanopt_amd.devvec import DeviceVector

pytestmark = pytest.mark.gpu

CAP = 64 << 20
ONE_ITEM = x_shape._case(True)                                      # (not in poison_ops.CASES: it selects the other kernel by a hook of the build)
CASES = po.CASES + [ONE_ITEM]
PAST_ONE_PASS = 2 * 4096 * 256 + 1537                               # test_reductions_exact_gpu.py: more than one grid-stride pass of a 4096-workgroup kernel
VEC_SIZES = tuple(po.VEC_SIZES) + (31, 32, 33, PAST_ONE_PASS)       # slack 8, 0 and 248 bytes among them
BOTH_KNOBS = ("kdyn-16-Final-Discrete", "sh23-54-Discrete", "shb23-127", "pois-18x15-s0")
BAD_VALUES = ("100", "0", "-4096", "4096.0", "", " 4096", "2147483648")


def zone_bytes(requested, cap=CAP):
    """The rule of guard.hpp: clamp(round_up(requested, 256), 4096, cap)."""
    return min(max((requested + 255) // 256 * 256, 4096), cap)


def guard_word(region, i):
    """Word i of the front zone (region 1) or of slack + back zone (region 2): guard::word."""
    return (0xA5 << 56) | ((0xC0 | region) << 48) | ((i * 0x9E3779B97F4B + 0x6A09E667F3BD) & 0xFFFFFFFFFFFF)


@pytest.fixture
def guard(monkeypatch):
    """SMO_GUARD set for the test, with a clean tally before and a drained pool after."""
    gc.collect()
    devvec.release_pool()
    _capi.guard_report()
    monkeypatch.setenv("SMO_GUARD", str(CAP))
    yield
    monkeypatch.delenv("SMO_GUARD", raising=False)
    gc.collect()
    devvec.release_pool()
    _capi.guard_report()


# ---- (a) every path -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_no_path_writes_outside_its_blocks(case, monkeypatch):
    monkeypatch.delenv("SMO_GUARD", raising=False)
    gc.collect()
    _capi.guard_report()
    ref, ref_paths = po.run(case, None, monkeypatch)
    assert _capi.guard_report()[:2] == (0, 0)                        # unset: nothing is guarded, nothing is counted
    monkeypatch.setenv("SMO_GUARD", str(CAP))
    try:
        got, paths = po.run(case, None, monkeypatch)                 # drops the contexts and releases the vector pool before it returns
    finally:
        monkeypatch.delenv("SMO_GUARD", raising=False)
    gc.collect()
    checked, damaged, first = _capi.guard_report()
    assert damaged == 0, "%d of %d blocks damaged, the first: %s" % (damaged, checked, first)
    assert checked >= 1
    assert paths == ref_paths, "SMO_GUARD: path indicators %s instead of %s" % (paths, ref_paths)
    assert len(got) == len(ref), "SMO_GUARD: %d values instead of %d" % (len(got), len(ref))
    assert _first_difference(ref, got) is None, "SMO_GUARD: %s" % _first_difference(ref, got)


# ---- (b) device vectors ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", VEC_SIZES)
def test_device_vector_algebra_under_the_guard(n, guard):
    for k, (got, want) in enumerate(po.vector_algebra(n)):
        assert np.array_equal(got, want), k
    checked, damaged, first = _capi.guard_report()                   # the vectors vector_algebra dropped were checked by their frees
    assert damaged == 0, first
    assert checked >= 6


def test_axpby_on_odd_views_under_the_guard(guard):
    """The one-element-per-lane kernel ends exactly at the last requested element of its output, whose block has no slack (n = 32 * k)."""
    for n in (32, 1024, 3 * 4096 * 256):
        rs = np.random.RandomState(n % 1000)
        x, y = rs.standard_normal(n), rs.standard_normal(n)
        X, Y, O = DeviceVector.from_numpy(x), DeviceVector.from_numpy(y), DeviceVector.from_numpy(np.zeros(n))
        a, b = 1.25, -0.3333333333333333
        _capi._check(_capi.lib().smo_vec_axpby(0, n - 1, a, C.c_void_p(X.ptr + 8), b, C.c_void_p(Y.ptr + 8), C.c_void_p(O.ptr + 8)))
        out = O.numpy()
        assert out[0] == 0. and np.array_equal(out[1:], a * x[1:] + b * y[1:])
        _capi._check(_capi.lib().smo_vec_axpby(0, n - 1, a, C.c_void_p(X.ptr + 8), b, None, C.c_void_p(O.ptr)))      # mixed alignment, no y
        out = O.numpy()
        assert np.array_equal(out[:n - 1], a * x[1:]) and out[n - 1] == a * x[n - 1] + b * y[n - 1]
        checked, damaged, first = _capi.guard_report()               # X, Y, O alive (and what the round before gave back)
        assert damaged == 0, first
        assert checked >= 3
        del X, Y, O


def _kdyn_small():
    from spheremanopt_amd import kdyn
    dom = kdyn.KDynDomain(8)
    members = [po.kd_inputs(12, b) for b in range(2)]
    X = [np.concatenate([m[0][comp] for m in members]) for comp in range(2)]
    return dom, dom.context((0.7, 1.3), po.kd_dt(12), 3, "Final", batch=2), X


def _sh23_small():
    from spheremanopt_amd import sh23
    import band_ops as bo
    dom = sh23.SH23Domain(54)
    return dom, dom.context(bo.sh23_dt(54), po.SH_HZ, batch=3), [po.white_inputs("sh23", 54, 3)[0]]


def _shb23_small():
    from spheremanopt_amd import shb23
    import band_ops as bo
    dom = shb23.SHBDomain(127)
    return dom, dom.context(bo.shb23_dt(127, False), po.SHB_N), [po.white_inputs("shb23", 127)[0]]


def _pois_small():
    from spheremanopt_amd import poiseuille as pz
    dom = pz.PoiseuilleDomain(18, 15)
    return dom, dom.context(po.PZ_RE, po.PZ_RI, po.PZ_N, po.PZ_DT, 0, po.PZ_PR, po.PZ_DELTA), [po.white_inputs("pois", (18, 15))[0]]


SMALL = {"kdyn": _kdyn_small, "sh23": _sh23_small, "shb23": _shb23_small, "pois": _pois_small}


@pytest.mark.parametrize("family", sorted(SMALL))
def test_dev_entry_points_write_inside_the_vectors_they_are_given(family, guard):
    """forward_dev / adjoint_dev (every family), hessvec_dev (SH23) and combine_dev (the batched KDyn and SH23 contexts) on DeviceVectors under
    the guard: the bits of the host entry points, and no zone of any vector or context buffer damaged."""
    dom, ctx, X = SMALL[family]()
    try:
        n = ctx.vec_len * ctx.batch
        J = ctx.forward(X)
        g = ctx.adjoint(None, "Discrete")
        dX = [DeviceVector.from_numpy(x) for x in X]
        dG = [DeviceVector(n) for _ in range(ctx.ngrad)]
        assert np.array_equal(ctx.forward_dev(dX), J)
        ctx.adjoint_dev(dX, dG, "Discrete")
        for c in range(ctx.ngrad):
            assert np.array_equal(dG[c].numpy(), g[c]), c
        if family == "sh23":
            (HV,), dJ = ctx.hessvec([X[0][::-1].copy()])
            dV, dH = DeviceVector.from_numpy(X[0][::-1].copy()), DeviceVector(n)
            _, dJ_dev = ctx.hessvec_dev([dV], [dH])
            assert np.array_equal(dH.numpy(), HV) and np.array_equal(dJ_dev, dJ)
            del dV, dH
        if family in ("kdyn", "sh23"):
            Cm = np.random.RandomState(17).standard_normal((ctx.batch, ctx.batch))
            dO = DeviceVector(n)
            ctx.combine_dev(Cm, dX[0], dO)
            assert np.array_equal(dO.numpy(), ctx.combine(Cm, X[0]))
            del dO
        checked, damaged, first = _capi.guard_report(ctx)            # the context's live blocks and the live vectors, now
        assert damaged == 0, first
        assert checked >= len(dX) + len(dG) + 1
        del dX, dG
    finally:
        dom.drop_contexts()
    gc.collect()
    checked, damaged, first = _capi.guard_report()                   # and again as they were given back
    assert damaged == 0, first
    assert checked >= 1


# ---- (c) the detector sees a device write --------------------------------------------------------------------------------------------------------------
def test_a_store_into_a_zone_is_reported_with_zone_and_offset(guard):
    n = 33
    req, rounded = 8 * n, 512
    Z = zone_bytes(req)
    assert Z == 4096 and rounded - req == 248
    V = DeviceVector.from_numpy(np.arange(1., n + 1.))
    S = DeviceVector(2)                                              # the source of the stores
    assert V.ptr % 256 == 0
    lo, hi = V.ptr - Z, V.ptr + rounded + Z                          # what the library allocated around V: [front zone][block][slack][back zone]
    targets = (("slack", "end+0,", V.ptr + req, 2, 0),               # (name, offset in the report, address, region, word of the region)
               ("back zone", "end+248,", V.ptr + rounded, 2, 248 // 8),
               ("back zone", "end+%d," % (248 + Z - 8), V.ptr + rounded + Z - 8, 2, (248 + Z - 8) // 8),
               ("front zone", "start-8,", V.ptr - 8, 1, Z // 8 - 1),
               ("front zone", "start-%d," % Z, V.ptr - Z, 1, 0))
    assert _capi.guard_report()[:2] == (2, 0)
    for zone, where, addr, region, word in targets:
        # a value that differs from the pattern in every byte (a finite double: 1.0 * value keeps its bits), so the first damaged byte is the word's first
        value = np.array([guard_word(region, word) ^ 0xFFFFFFFFFFFFFFFF, 0], dtype=np.uint64).view(np.float64)
        assert np.isfinite(value[0])
        _capi._check(_capi.lib().smo_vec_upload(0, S.ptr, value.ctypes.data, 2))
        assert lo <= addr and addr + 8 <= hi and not (V.ptr <= addr < V.ptr + req), "the target must lie in a zone or the slack of V"
        assert addr % 8 == 0
        _capi._check(_capi.lib().smo_vec_axpby(0, 1, 1.0, C.c_void_p(S.ptr), 0.0, None, C.c_void_p(addr)))
        checked, damaged, first = _capi.guard_report()
        assert (checked, damaged) == (2, 1), (zone, where, first)
        assert first.startswith("smo_vec_alloc, %d bytes requested: %s, first damaged byte at %s 1 damaged 8-byte word(s)" % (req, zone, where)), first
        assert _capi.guard_report() == (2, 0, ""), "the report patterns a damaged block again"
    assert np.array_equal(V.numpy(), np.arange(1., n + 1.))          # and the block itself was never touched
    # two words at once, in two zones: still one damaged block, the front zone named first, both words counted
    for addr in (V.ptr - 16, V.ptr + rounded + 64):
        assert lo <= addr and addr + 8 <= hi
        _capi._check(_capi.lib().smo_vec_axpby(0, 1, 1.0, C.c_void_p(S.ptr), 0.0, None, C.c_void_p(addr)))
    checked, damaged, first = _capi.guard_report()
    assert (checked, damaged) == (2, 1) and "front zone, first damaged byte at start-16, 2 damaged" in first, first
    del V, S
    gc.collect()
    assert _capi.guard_report()[:2] == (4, 0)                        # checked by their frees, and once more in the pool: intact


def test_a_block_from_the_free_list_is_patterned_for_its_new_length(guard):
    """n = 33 and n = 64 share a 512-byte block: the slack of the first owner (words 33 .. 63) is the second owner's data, and the other way round."""
    A = DeviceVector.from_numpy(np.arange(64.))
    ptr = A.ptr
    del A
    B = DeviceVector.from_numpy(np.arange(33.))
    assert B.ptr == ptr
    assert _capi.guard_report()[:2] == (2, 0)                        # the free of A and B alive
    slack0 = B.ptr + 8 * 33
    assert B.ptr <= slack0 and slack0 + 8 <= B.ptr + 512 + zone_bytes(8 * 33)
    _capi._check(_capi.lib().smo_vec_axpby(0, 1, 1.0, C.c_void_p(B.ptr), 0.0, None, C.c_void_p(slack0)))      # what A could write, B may not
    checked, damaged, first = _capi.guard_report()
    assert (checked, damaged) == (1, 1) and "264 bytes requested: slack, first damaged byte at end+" in first, first
    del B


# ---- (d) the knob acts at the DevPool site and changes nothing else ----------------------------------------------------------------------------------------
def _geometry(family):
    dom, ctx, _ = SMALL[family]()
    try:
        n = C.c_size_t()
        _capi._check(_capi.lib().smo_stack_bytes(ctx._h, C.byref(n)))
        live = _capi.guard_report(ctx)
        return (n.value, ctx.stack_bytes, ctx.vec_len, ctx.snapshot_len) + tuple(ctx.get(k) for k in range(7)) + devvec.pool_bytes(), live
    finally:
        dom.drop_contexts()


@pytest.mark.parametrize("family", sorted(SMALL))
def test_the_knob_guards_context_buffers_and_moves_no_byte_count(family, monkeypatch):
    gc.collect()
    devvec.release_pool()
    monkeypatch.delenv("SMO_GUARD", raising=False)
    _capi.guard_report()
    plain, live = _geometry(family)
    assert live == (0, 0, "") and _capi.guard_report() == (0, 0, "")              # unset: nothing is guarded, nothing is counted
    monkeypatch.setenv("SMO_GUARD", str(CAP))
    try:
        guarded, live = _geometry(family)
    finally:
        monkeypatch.delenv("SMO_GUARD")
    assert guarded == plain
    assert live[0] >= 1 and live[1] == 0, live                       # no device vector is in play: these are the context's own blocks
    checked, damaged, first = _capi.guard_report()                   # ... each checked again when the context gave it back
    assert damaged == 0, first
    assert checked >= live[0]


def test_guarded_vectors_keep_their_alignment_and_their_byte_counts(monkeypatch):
    gc.collect()
    devvec.release_pool()
    _capi.guard_report()
    sizes = (1, 31, 32, 33, 511, 512, 513, 1001, 70001)

    def measure():
        vs = [DeviceVector(n) for n in sizes]
        out = ([v.ptr % 256 for v in vs], devvec.pool_bytes())
        del vs
        gc.collect()
        out += (devvec.pool_bytes(),)
        devvec.release_pool()
        return out + (devvec.pool_bytes(),)

    monkeypatch.delenv("SMO_GUARD", raising=False)
    plain = measure()
    monkeypatch.setenv("SMO_GUARD", str(CAP))
    try:
        guarded = measure()
        monkeypatch.setenv("SMO_GUARD", "4096")                      # the smallest cap: every zone is 4096 bytes
        smallest = measure()
    finally:
        monkeypatch.delenv("SMO_GUARD")
    assert plain[0] == [0] * len(sizes) and plain[3] == (0, 0)
    assert guarded == plain and smallest == plain
    assert _capi.guard_report()[:2] == (2 * len(sizes), 0)           # every free of a guarded vector was a check


def test_a_guarded_block_is_not_handed_out_when_the_knob_is_unset(monkeypatch):
    """Whether a block is guarded is kept with the block: the free list holds both kinds apart, and a guarded block freed after the knob went
    away is still checked."""
    gc.collect()
    devvec.release_pool()
    _capi.guard_report()
    monkeypatch.setenv("SMO_GUARD", str(CAP))
    A = DeviceVector(33)
    ptr = A.ptr
    monkeypatch.delenv("SMO_GUARD")
    del A                                                            # checked although the knob is gone
    assert _capi.guard_report()[:2] == (2, 0)                        # its free, and the pooled block once more
    B = DeviceVector(33)
    assert B.ptr != ptr and devvec.pool_bytes() == (512, 512)
    monkeypatch.setenv("SMO_GUARD", str(CAP))
    A = DeviceVector(33)
    assert A.ptr == ptr and devvec.pool_bytes() == (1024, 0)
    monkeypatch.delenv("SMO_GUARD")
    del A, B
    devvec.release_pool()
    _capi.guard_report()


@pytest.mark.parametrize("case", [c for c in po.CASES if c["id"] in BOTH_KNOBS], ids=BOTH_KNOBS)
def test_guard_and_poison_together(case, monkeypatch):
    """SMO_POISON fills the requested bytes only: the zones survive it, and the bits are those of the run with neither knob."""
    monkeypatch.delenv("SMO_GUARD", raising=False)
    ref, ref_paths = po.run(case, None, monkeypatch)
    _capi.guard_report()
    monkeypatch.setenv("SMO_GUARD", str(CAP))
    try:
        got, paths = po.run(case, 255, monkeypatch)
        fresh = DeviceVector(33)                                     # and a vector nobody wrote reads back as the fill, slack and zones intact
        monkeypatch.setenv("SMO_POISON", "255")
        filled = DeviceVector(33)
        assert po.same_bits(filled.numpy(), po.fill_pattern(255, 33))
        del fresh, filled
    finally:
        monkeypatch.delenv("SMO_GUARD", raising=False)
        monkeypatch.delenv("SMO_POISON", raising=False)
    gc.collect()
    devvec.release_pool()
    checked, damaged, first = _capi.guard_report()
    assert damaged == 0, first
    assert checked >= 3
    assert paths == ref_paths and len(got) == len(ref)
    assert _first_difference(ref, got) is None, "SMO_GUARD + SMO_POISON=255: %s" % _first_difference(ref, got)


# ---- (e) a bad value ------------------------------------------------------------------------------------------------------------------------------------
def test_a_value_that_is_no_cap_is_an_argument_error(monkeypatch):
    gc.collect()
    devvec.release_pool()
    _capi.guard_report()
    for bad in BAD_VALUES:
        monkeypatch.setenv("SMO_GUARD", bad)
        with pytest.raises(_capi.SmoError) as e:
            DeviceVector(4)
        assert e.value.code == 1 and "SMO_GUARD" in str(e.value), bad
        with pytest.raises(_capi.SmoError) as e:
            _capi.Context(_capi.SMO_SH23, 16, (0., 12. * np.pi), 0.1, 2, -0.3)
        assert e.value.code == 1 and "SMO_GUARD" in str(e.value), bad
    monkeypatch.delenv("SMO_GUARD")
    assert DeviceVector(4).numpy().shape == (4,)
    gc.collect()
    devvec.release_pool()
    assert _capi.guard_report() == (0, 0, "")
