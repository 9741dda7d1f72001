"""Write-through stores on the hand-over streams of the KDyn time loop change no bit (csrc/kdyn.hip: SMO_KD_WT, st_cplx).

The y passes and the update kernels store the streams they hand to the next kernel — Ty, Tz, the new state, the next step's Tz — either
with plain stores or with 16-byte write-through stores, one policy bit per stream, chosen per grid at build time (Shape<L>::WT).  SMO_KD_WT=0, read once when a context is created, selects plain stores on every stream; smo_get key 7 reports the streams in
force.  A store flavour moves the same value to the same address, so every number a solve returns must be equal bit for bit: np.array_equal
on J, dJ/dB0 and dJ/dU and on the rest of poison_ops' sequence (inner products, every snapshot, a second input on the same context, the first
input again).

Shapes, the smallest that reach every changed store:
  Npts = 8   (G = 12): the plane layout of Ty, whole solves replayed from captured graphs; 5 steps, Final and Integrated cost;
  Npts = 16  (G = 24): z-block-major Ty, three z blocks; 5 steps;
  Npts = 128 (G = 192), 3 steps: the flagship instantiation with the two-wave adjoint x pass, and its one-item shape (SMO_KD_ADJ_SEQ_ITEMS=1);
  Npts = 8:  batch 2 (the member offset in the store's base), ckpt = 2 with 5 steps (a replayed window writes the same slots twice), a
             frozen-velocity context (no Ty stack: every Ty goes to the work buffer);
  one case with every allocation filled first (SMO_POISON=255), and one between guard zones (SMO_GUARD, cap 64 MiB): a store through a buffer
  resource whose range is left at the maximum is not clipped, so an overrun would land in a zone and be reported — damaged must be 0.

A case whose grid has no write-through stream in this build has nothing to compare and skips, saying so.
"""
import gc

import numpy as np
import pytest

import poison_ops as po
from spheremanopt_amd import _capi

pytestmark = pytest.mark.gpu

HOOK = "SMO_KD_WT"
CAP = 64 << 20                                  # test_guard_gpu.py's cap


def _kd(N, variant, n=5, cost="Final", adj="Discrete", env=None, **kw):
    c = po._case("kdyn", N, variant, n=n, cost=cost, adj=adj, env=dict(env or {}), **kw)
    c["id"] = po.case_id(c)
    return c


CASES = [
    _kd(8, "graph", replays=True),
    _kd(8, "graph", cost="Integrated", replays=True),
    _kd(16, "plain"),
    _kd(128, "two-wave", n=3),
    _kd(128, "one item per thread", n=3, env={"SMO_KD_ADJ_SEQ_ITEMS": "1"}),
    _kd(8, "batch=2", batch=2, rm=(0.7, 1.3)),
    _kd(8, "ckpt=2", ckpt=2),
    _kd(8, "frozen_U", frozen=True, keep=True),
]
IDS = [c["id"] for c in CASES]

_MASK, _REF = {}, {}


def _streams(N, monkeypatch):
    """smo_get key 7 of a default context at this grid: the write-through streams the build adopted there."""
    if N not in _MASK:
        from spheremanopt_amd import kdyn
        monkeypatch.delenv(HOOK, raising=False)
        dom = kdyn.KDynDomain(N)
        try:
            _MASK[N] = int(dom.context(po.KD_RM, po.kd_dt(3 * N // 2), 1, "Final").get(7))
        finally:
            dom.drop_contexts()
    return _MASK[N]


def _need_streams(case, monkeypatch):
    if _streams(case["size"], monkeypatch) == 0:
        pytest.skip("this build stores no stream write-through at G = %d: both policies are the same kernels" % (3 * case["size"] // 2))


def _plain(case, monkeypatch):
    """The case with SMO_KD_WT=0: computed once, shared by the tests below, never written to."""
    if case["id"] not in _REF:
        c = dict(case, env=dict(case["env"], **{HOOK: "0"}))
        values, paths = po.run(c, None, monkeypatch)
        for v in values:
            v.setflags(write=False)
        _REF[case["id"]] = (values, paths)
    return _REF[case["id"]]


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


def test_the_knob_switches_every_stream_off(monkeypatch):
    """SMO_KD_WT=0 leaves no stream write-through at any grid, and the run-time-length kernels never have one."""
    from spheremanopt_amd import kdyn
    for N, env in ((8, {HOOK: "0"}), (128, {HOOK: "0"}), (8, {"SMO_KD_ANY": "1"}), (22, {})):
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        dom = kdyn.KDynDomain(N)
        try:
            assert dom.context(po.KD_RM, po.kd_dt(3 * N // 2), 1, "Final").get(7) == 0, (N, env)
        finally:
            dom.drop_contexts()
            for name in env:
                monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_write_through_equals_plain_stores_bit_for_bit(case, monkeypatch):
    _need_streams(case, monkeypatch)
    ref = _plain(case, monkeypatch)
    for k, v in enumerate(ref[0]):
        assert np.all(np.isfinite(v)), "value %d of %d is not finite" % (k, len(ref[0]))
    assert float(np.linalg.norm(ref[0][1])) > 0
    monkeypatch.delenv(HOOK, raising=False)
    got = po.run(case, None, monkeypatch)
    _assert_same(ref, got, "write-through streams %d against %s=0" % (_streams(case["size"], monkeypatch), HOOK))


@pytest.mark.parametrize("case", [CASES[2]], ids=[IDS[2]])
def test_write_through_does_not_depend_on_what_memory_held(case, monkeypatch):
    _need_streams(case, monkeypatch)
    ref = _plain(case, monkeypatch)
    monkeypatch.delenv(HOOK, raising=False)
    got = po.run(case, 255, monkeypatch)
    _assert_same(ref, got, "SMO_POISON=255")


@pytest.mark.parametrize("case", [CASES[2]], ids=[IDS[2]])
def test_write_through_stores_stay_inside_their_blocks(case, monkeypatch):
    _need_streams(case, monkeypatch)
    ref = _plain(case, monkeypatch)
    monkeypatch.delenv(HOOK, raising=False)
    gc.collect()
    _capi.guard_report()
    monkeypatch.setenv("SMO_GUARD", str(CAP))
    try:
        got = po.run(case, None, monkeypatch)                        # drops the contexts and releases the vector pool before it returns
    finally:
        monkeypatch.delenv("SMO_GUARD", raising=False)
    gc.collect()
    checked, damaged, first = _capi.guard_report()
    assert damaged == 0, "%d of %d blocks damaged, the first: %s" % (damaged, checked, first)
    assert checked >= 1
    _assert_same(ref, got, "SMO_GUARD")
