"""The two workgroup shapes of the sequential adjoint x pass give the same bits (csrc/kdyn.hip, SMO_X_SEQ_ITEMS; DESIGN.md section 4, "Tile shapes").

At G = 192 (Npts = 128) the pass runs as two-wave workgroups, two middle-section items (j, line pair) per thread, four tiles per CU; the
one-item-per-thread kernel (four waves, three tiles per CU) is built beside it and SMO_KD_ADJ_SEQ_ITEMS=1, read once when a context is
created, selects it.  Tile, layout, butterflies, twiddles, cross products and the order of the running-sum addition are the same, so every
number a solve returns must be equal bit for bit: np.array_equal on J, dJ/dB0 and dJ/dU, and on the rest of poison_ops' sequence (inner
products, every snapshot, a second input on the same context, the first input again).  N_ITERS = 3: the running sum of omega x B_f is
added to more than once.  The same run with every allocation filled first (SMO_POISON = 0xFF, 0x3F, as test_poison_gpu.py does) must give
those bits again: nothing the new shape reads — the tile buffer in the LDS, Ty, the running sum — may be something it did not write.

Why G = 192 is the smallest grid here: the shape needs a tile of 256 middle-section items ((T / 2) * G / 3 with T = 8 points) for 128 threads
to hold two each.  G = 96 (Npts = 64, the nearest length with a radix-2 stage) has 128 items per tile: a 128-thread workgroup there holds one
item per thread and has no two-item indexing to get wrong, and a 64-thread workgroup is a different shape (one wave, no barrier partner),
which is not built.  The only other tuned length with 256 items is G = 384 (half tiles), where the shape spills and is not enabled
(profiles/r15_kdyn_adj_x_two_wave_resources.txt); every length without the shape runs the kernel it ran before, which the existing suite
covers.
"""
import numpy as np
import pytest

import poison_ops as po

pytestmark = pytest.mark.gpu

N, N_ITERS = 128, 3
HOOK = "SMO_KD_ADJ_SEQ_ITEMS"


def _case(one_item):
    c = po._case("kdyn", N, "one item per thread" if one_item else "two-wave", n=N_ITERS, cost="Final", adj="Discrete",
                 env={HOOK: "1"} if one_item else {})
    c["id"] = po.case_id(c)
    return c


_REF = {}


def _two_wave_unset(monkeypatch):
    """The default shape with SMO_POISON unset: computed once, shared by the tests below, never written to."""
    if "ref" not in _REF:
        monkeypatch.delenv(HOOK, raising=False)
        values, paths = po.run(_case(False), None, monkeypatch)
        for v in values:
            v.setflags(write=False)
        _REF["ref"] = (values, paths)
    return _REF["ref"]


def _assert_same(ref, got, what):
    (rv, rp), (gv, gp) = ref, got
    assert gp == rp, "%s: path indicators %s instead of %s" % (what, gp, rp)
    assert len(gv) == len(rv), "%s: %d values instead of %d" % (what, len(gv), len(rv))
    names = ["J", "dJ/dB0", "dJ/dU"]
    for k, (r, g) in enumerate(zip(rv, gv)):
        name = names[k] if k < 3 else "value %d of the sequence" % k
        assert r.shape == g.shape, (what, name)
        if not np.array_equal(r, g):
            bad = np.flatnonzero(r.reshape(-1) != g.reshape(-1))
            raise AssertionError("%s: %s differs in %d of %d entries, the first at flat index %d: %r instead of %r" % (
                what, name, len(bad), r.size, bad[0], g.reshape(-1)[bad[0]], r.reshape(-1)[bad[0]]))


def test_reference_run_is_finite(monkeypatch):
    values, _ = _two_wave_unset(monkeypatch)
    assert len(values) >= 3
    for k, v in enumerate(values):
        assert np.all(np.isfinite(v)), "value %d of %d is not finite" % (k, len(values))
    assert float(np.linalg.norm(values[1])) > 0 and float(np.linalg.norm(values[2])) > 0


def test_two_wave_shape_equals_one_item_shape_bit_for_bit(monkeypatch):
    ref = _two_wave_unset(monkeypatch)
    got = po.run(_case(True), None, monkeypatch)
    _assert_same(ref, got, "%s=1" % HOOK)


@pytest.mark.parametrize("fill", po.FILLS[2:], ids=po.FILL_IDS[2:])
def test_two_wave_shape_does_not_depend_on_what_memory_held(fill, monkeypatch):
    ref = _two_wave_unset(monkeypatch)
    monkeypatch.delenv(HOOK, raising=False)
    got = po.run(_case(False), fill, monkeypatch)
    _assert_same(ref, got, "SMO_POISON=%d" % fill)


@pytest.mark.parametrize("fill", po.FILLS[2:3], ids=po.FILL_IDS[2:3])
def test_one_item_shape_under_a_fill_equals_the_two_wave_shape(fill, monkeypatch):
    """Both at once: the other kernel and other memory contents, the same bits."""
    ref = _two_wave_unset(monkeypatch)
    got = po.run(_case(True), fill, monkeypatch)
    _assert_same(ref, got, "%s=1, SMO_POISON=%d" % (HOOK, fill))
