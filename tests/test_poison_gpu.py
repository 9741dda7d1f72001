"""No result may depend on what device memory held before the solve (cases, fills, sequence and runner: poison_ops.py).

Every case runs four times on a fresh domain and context: with SMO_POISON unset and with every allocation filled with 0x00, 0xFF and 0x3F.
(a) every value of the unset run is finite; (b) each filled run equals the unset run bit for bit, arrays with np.array_equal and in their
order of production, so that the first differing quantity names the step (forward value, gradient component, <X, g>, snapshot, second
input, first input again); and the path indicators (ctx.get) are equal, so that the fill did not move the case onto another path.  A
condition, not a tolerance: the library promises fixed summation orders and no floating-point atomics.

The device vectors: their algebra equals NumPy's under every fill, and a vector nobody wrote reads back as the fill byte in every position
— a fresh block, one taken back from the free list, and a pinned host block — which is what proves that the knob acts at both device
allocation sites (they share one helper) and at the host one.

On an MI355X every case is bit-identical under all three fills (143 tests, 22.8 s). That the cases bite was shown on scratch builds with
one line removed (HISTORY.md): without KDyn's hipMemsetAsync(d_acc) the case kdyn-16-Final-Discrete fails under 0xFF (dJ/dU NaN) and 0x3F
(39578 of 41472 entries of dJ/dU), without Poiseuille's hipMemsetAsync(d_stack) the case pois-24x24-s0 fails under 0xFF (NaN) and 0x3F
(every gradient entry); both pass under 0x00, and the ordinary oracle tests of those sizes pass on both builds in a fresh process.
"""
import gc

import numpy as np
import pytest

import poison_ops as po
from spheremanopt_amd import _capi, devvec
from spheremanopt_amd.devvec import DeviceVector

pytestmark = pytest.mark.gpu


def _first_difference(ref, got):
    for k, (r, g) in enumerate(zip(ref, got)):
        if r.shape != g.shape or not np.array_equal(r, g):
            bad = np.flatnonzero(np.asarray(r).reshape(-1) != np.asarray(g).reshape(-1)) if r.shape == g.shape else []
            return "value %d of %d (shape %s): %d entries differ, the first at flat index %s: %r instead of %r" % (
                k, len(ref), r.shape, len(bad), bad[0] if len(bad) else "-", g.reshape(-1)[bad[0]] if len(bad) else None,
                r.reshape(-1)[bad[0]] if len(bad) else None)
    return None


@pytest.mark.parametrize("case", po.CASES, ids=[c["id"] for c in po.CASES])
def test_results_do_not_depend_on_what_memory_held(case, monkeypatch):
    ref, ref_paths = po.run(case, None, monkeypatch)
    for k, v in enumerate(ref):
        assert np.all(np.isfinite(v)), "unset run: value %d of %d is not finite" % (k, len(ref))
    problems = []                                                    # every fill is run and reported, not only the first that differs
    for fill, name in zip(po.FILLS[1:], po.FILL_IDS[1:]):
        got, paths = po.run(case, fill, monkeypatch)
        if paths != ref_paths:
            problems.append("SMO_POISON=%s: path indicators %s instead of %s" % (name, paths, ref_paths))
        if len(got) != len(ref):
            problems.append("SMO_POISON=%s: %d values instead of %d" % (name, len(got), len(ref)))
        elif _first_difference(ref, got) is not None:
            problems.append("SMO_POISON=%s: %s" % (name, _first_difference(ref, got)))
        del got
    del ref
    gc.collect()
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("n", po.VEC_SIZES)
@pytest.mark.parametrize("fill", po.FILLS, ids=po.FILL_IDS)
def test_device_vector_algebra_equals_numpy_under_every_fill(fill, n, monkeypatch):
    po.set_fill(monkeypatch, fill)
    try:
        for k, (got, want) in enumerate(po.vector_algebra(n)):
            assert np.array_equal(got, want), k
    finally:
        gc.collect()
        devvec.release_pool()


@pytest.mark.parametrize("n", po.VEC_SIZES)
@pytest.mark.parametrize("fill", po.FILLS[1:], ids=po.FILL_IDS[1:])
def test_a_vector_nobody_wrote_reads_back_as_the_fill(fill, n, monkeypatch):
    """Readback: a fresh block, a block from the free list whose last owner held other contents, a pinned host block.  (Unset: no
    assertion on content.)"""
    gc.collect()
    devvec.release_pool()
    po.set_fill(monkeypatch, fill)
    want = po.fill_pattern(fill, n)
    try:
        fresh = DeviceVector(n)
        assert po.same_bits(fresh.numpy(), want)
        live, pooled = devvec.pool_bytes()
        other = DeviceVector.from_numpy(np.arange(1., n + 1.))
        ptr = other.ptr
        del other                                                    # back to the free list with 1 .. n in it
        held = devvec.pool_bytes()[1]
        assert held > pooled
        again = DeviceVector(n)
        assert again.ptr == ptr and devvec.pool_bytes()[1] < held    # the very block, out of the free list
        assert po.same_bits(again.numpy(), want)
        assert po.same_bits(_capi.pinned_empty(n), want)
        del fresh, again
    finally:
        gc.collect()
        devvec.release_pool()


def test_a_value_that_is_no_byte_is_an_argument_error(monkeypatch):
    for bad in ("256", "-1", "0x3F", "1.5", "", " 7", "banded"):
        monkeypatch.setenv("SMO_POISON", bad)
        with pytest.raises(_capi.SmoError) as e:
            DeviceVector(4)
        assert e.value.code == 1 and "SMO_POISON" in str(e.value)
        with pytest.raises(_capi.SmoError) as e:
            _capi.pinned_empty(4)
        assert e.value.code == 1
        with pytest.raises(_capi.SmoError) as e:
            _capi.Context(_capi.SMO_SH23, 16, (0., 12. * np.pi), 0.1, 2, -0.3)
        assert e.value.code == 1 and "SMO_POISON" in str(e.value)
    monkeypatch.delenv("SMO_POISON")
    assert DeviceVector(4).numpy().shape == (4,)
    gc.collect()
    devvec.release_pool()
