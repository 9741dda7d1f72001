"""No result may depend on what the LDS held when a kernel was launched (SMO_POISON_LDS: csrc/lds_poison.hip, the hook of csrc/smo_common.hpp;
the sibling for the LDS of test_poison_gpu.py and test_guard_gpu.py).

LDS is not cleared between dispatches: a workgroup starts with what the last workgroup on its CU left, which in a test process is the previous
kernel of the same solve — finite, often zero.  A padding row, the tail of a ragged tile, an unpaired last line or a slot of a run-time plan
that is read but never written passes every other test, and so does such a read multiplied by a zero operand.  With SMO_POISON_LDS=<byte>
every launch of the library is preceded on its stream by a fill dispatch that leaves that byte in every byte of every CU's LDS.

(a) every case of poison_ops.CASES, and the one-item shape of the adjoint x pass at 128^3, runs with the knob unset, with 255 (every word a
    NaN) and with 63 (the finite 4.8e-4, which a comparison or a select that swallows a NaN still shifts): the bits of the unset run in order
    of production, the same path indicators, fills_launched == launches_hooked >= 1 under the knob and 0 / 0 without it.  A condition, not a
    tolerance; no case is skipped and no launch is exempt (test_lds_poison_cpu.py: no launch outside the hook).
(b) the fill reaches what a kernel sees: under 255 and 63 the probe (smo_lds_probe: workgroups that read their LDS without writing it) finds
    the fill word in every word of 1 KiB, 40 KiB, 64 KiB and 163 840 bytes of LDS on grids of 1x and 4x the CU count; unset it reports 0 fills.
(c) device vectors under the knob: the algebra equals NumPy's, also one element per lane on odd views.
(d) the knob changes nothing else: byte counts and path indicators; one case per family under SMO_POISON_LDS=255, SMO_POISON=255 and
    SMO_GUARD together gives the unset run's bits and no damaged block.
(e) a value that is no byte is an argument error at context creation and at smo_vec_alloc.

Not seen by this suite: DESIGN.md section 7.

On an MI355X: 164 tests in 32.4 s, every case bit-identical under both fills and every probed word equal to the fill (up to 20 971 520 words:
1024 workgroups of 163 840 bytes); the slowest are kdyn-256-Final-Discrete (5.8 s for its three runs), shb23-1023 (3.3 s), kdyn-128 and
shb23-512-batch=3 (0.7 s each).
"""
import ctypes as C
import gc

import numpy as np
import pytest

import poison_ops as po
import test_guard_gpu as tg
from test_poison_gpu import _first_difference
from spheremanopt_amd import _capi, devvec
from spheremanopt_amd.devvec import DeviceVector

pytestmark = pytest.mark.gpu

KNOB = "SMO_POISON_LDS"
FILLS = (255, 63)
CASES = po.CASES + [tg.ONE_ITEM]
PROBE_BYTES = (1 << 10, 40 << 10, 64 << 10, 163840)
PROBE_GRIDS = (1, 4)                                                # multiples of the CU count
BAD_VALUES = ("256", "-1", "1.0", "", " 7", "0x3F")


def fill_word(byte):
    """The 8-byte word the fill stores (csrc/lds_poison.hpp: fill_word)."""
    return 0x0101010101010101 * byte


def _cu_count():
    return _capi.device_cus(0)


def _take():
    """Read the knob as the environment has it now, take and reset the two counters of the hook: (fills, launches)."""
    return _capi.lds_probe()[2:]


# ---- (a) every path -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_no_path_reads_lds_it_did_not_write(case, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    gc.collect()
    _take()
    ref, ref_paths = po.run(case, None, monkeypatch)
    assert _take() == (0, 0)                                         # unset: no fill, and no launch took the hook's branch
    problems = []                                                    # both fills are run and reported, not only the first that differs
    for fill in FILLS:
        monkeypatch.setenv(KNOB, str(fill))
        try:
            got, paths = po.run(case, None, monkeypatch)
        finally:
            monkeypatch.delenv(KNOB, raising=False)
        fills, launches = _take()
        if not (fills == launches and launches >= 1):
            problems.append("%s=%d: %d fills for %d launches" % (KNOB, fill, fills, launches))
        if paths != ref_paths:
            problems.append("%s=%d: path indicators %s instead of %s" % (KNOB, fill, paths, ref_paths))
        if len(got) != len(ref):
            problems.append("%s=%d: %d values instead of %d" % (KNOB, fill, len(got), len(ref)))
        elif _first_difference(ref, got) is not None:
            problems.append("%s=%d: %s" % (KNOB, fill, _first_difference(ref, got)))
        del got
    del ref
    gc.collect()
    assert not problems, "\n".join(problems)


# ---- (b) the fill reaches what a kernel sees -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", PROBE_GRIDS)
@pytest.mark.parametrize("lds_bytes", PROBE_BYTES)
@pytest.mark.parametrize("fill", FILLS)
def test_the_probe_finds_the_fill_in_every_word(fill, lds_bytes, grid, monkeypatch):
    wgs = grid * _cu_count()
    monkeypatch.setenv(KNOB, str(fill))
    try:
        _take()
        words, equal, fills, launches = _capi.lds_probe(lds_bytes, wgs)
    finally:
        monkeypatch.delenv(KNOB, raising=False)
        _take()
    print("fill %d, %d bytes x %d workgroups: %d of %d words equal the fill" % (fill, lds_bytes, wgs, equal, words))
    assert words == wgs * lds_bytes // 8
    assert (fills, launches) == (1, 1)
    assert equal == words, "%d of %d probed words do not hold %#018x" % (words - equal, words, fill_word(fill))


def test_the_probe_reports_no_fill_when_the_knob_is_unset(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    _take()
    words, equal, fills, launches = _capi.lds_probe(1 << 10, _cu_count())
    assert words == _cu_count() * 128 and (fills, launches) == (0, 0)           # (nothing is asserted about what it read)
    assert _capi.lds_probe() == (0, 0, 0, 0)


# ---- (c) device vectors ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", tg.VEC_SIZES)
@pytest.mark.parametrize("fill", FILLS)
def test_device_vector_algebra_under_the_lds_fill(fill, n, monkeypatch):
    monkeypatch.setenv(KNOB, str(fill))
    try:
        _take()
        for k, (got, want) in enumerate(po.vector_algebra(n)):
            assert np.array_equal(got, want), k
        fills, launches = _take()
        assert fills == launches and launches >= 4
    finally:
        monkeypatch.delenv(KNOB, raising=False)
        gc.collect()
        devvec.release_pool()
        _take()


@pytest.mark.parametrize("fill", FILLS)
def test_axpby_on_odd_views_under_the_lds_fill(fill, monkeypatch):
    monkeypatch.setenv(KNOB, str(fill))
    try:
        _take()
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
            del X, Y, O
        assert _take() == (6, 6)
    finally:
        monkeypatch.delenv(KNOB, raising=False)
        gc.collect()
        devvec.release_pool()
        _take()


# ---- (d) the knob changes nothing else --------------------------------------------------------------------------------------------------------------
def _geometry(family):
    dom, ctx, _ = tg.SMALL[family]()
    try:
        n = C.c_size_t()
        _capi._check(_capi.lib().smo_stack_bytes(ctx._h, C.byref(n)))
        return (n.value, ctx.stack_bytes, ctx.vec_len, ctx.snapshot_len) + tuple(ctx.get(k) for k in range(7)) + devvec.pool_bytes()
    finally:
        dom.drop_contexts()


@pytest.mark.parametrize("family", sorted(tg.SMALL))
def test_the_knob_moves_no_byte_count_and_no_path(family, monkeypatch):
    gc.collect()
    devvec.release_pool()
    monkeypatch.delenv(KNOB, raising=False)
    plain = _geometry(family)
    monkeypatch.setenv(KNOB, "255")
    try:
        filled = _geometry(family)
    finally:
        monkeypatch.delenv(KNOB, raising=False)
        _take()
    assert filled == plain


@pytest.mark.parametrize("case", [c for c in po.CASES if c["id"] in tg.BOTH_KNOBS], ids=tg.BOTH_KNOBS)
def test_lds_fill_poison_and_guard_together(case, monkeypatch):
    for name in (KNOB, "SMO_GUARD"):
        monkeypatch.delenv(name, raising=False)
    gc.collect()
    devvec.release_pool()
    ref, ref_paths = po.run(case, None, monkeypatch)
    _capi.guard_report()
    assert _take() == (0, 0)
    monkeypatch.setenv("SMO_GUARD", str(tg.CAP))
    monkeypatch.setenv(KNOB, "255")
    try:
        got, paths = po.run(case, 255, monkeypatch)
    finally:
        monkeypatch.delenv("SMO_GUARD", raising=False)
        monkeypatch.delenv(KNOB, raising=False)
    gc.collect()
    devvec.release_pool()
    checked, damaged, first = _capi.guard_report()
    fills, launches = _take()
    assert damaged == 0, first
    assert checked >= 1
    assert fills == launches and launches >= 1
    assert paths == ref_paths and len(got) == len(ref)
    assert _first_difference(ref, got) is None, "%s + SMO_POISON + SMO_GUARD: %s" % (KNOB, _first_difference(ref, got))


# ---- (e) a bad value ------------------------------------------------------------------------------------------------------------------------------------
def test_a_value_that_is_no_byte_is_an_argument_error(monkeypatch):
    gc.collect()
    devvec.release_pool()
    for bad in BAD_VALUES:
        monkeypatch.setenv(KNOB, bad)
        with pytest.raises(_capi.SmoError) as e:
            DeviceVector(4)
        assert e.value.code == 1 and KNOB in str(e.value), bad
        with pytest.raises(_capi.SmoError) as e:
            _capi.Context(_capi.SMO_SH23, 16, (0., 12. * np.pi), 0.1, 2, -0.3)
        assert e.value.code == 1 and KNOB in str(e.value), bad
    monkeypatch.delenv(KNOB)
    assert DeviceVector(4).numpy().shape == (4,)
    gc.collect()
    devvec.release_pool()
    assert _take() == (0, 0)
