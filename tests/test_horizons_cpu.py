"""A time horizon of its own for every batch member (smo_set_horizons), the parts that need no GPU: both entry points are declared, exported and
bound; the Python front end refuses a bad N_ITERS sequence before any device call; and the premise of every test that compares members at
different horizons — J really depends on the horizon — holds on the oracles."""
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from parameter_cases import sh23_input
from spheremanopt_amd import _capi, kdyn, sh23
from test_kdyn_batch_gpu import _members


def test_entry_points_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smo.h")).read(), flags=re.S)
    for name, params in (("smo_set_horizons", ["ctx", "n_iters"]), ("smo_get_horizons", ["ctx", "n_iters"])):
        m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name, hdr)
        assert m, "include/smo.h does not declare %s" % name
        assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == params
        assert name in _capi.SIGNATURES and name in _capi.EXPORTS
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is _capi.C.c_int and len(argtypes) == len(params)
    body = re.search(r"typedef\s+struct\s+smo_config\s*\{(.*?)\}\s*smo_config\s*;", hdr, flags=re.S).group(1)
    assert len(re.findall(r"\b(\w+)\s*(?:,|;)", body)) == 17 == len(_capi.smo_config._fields_)      # the config keeps its fields
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(_capi.lib(), "smo_set_horizons") and hasattr(_capi.lib(), "smo_get_horizons")


class _NoDevice:
    """Stands in for _capi inside a problem module: any attempt to open a context is a test failure."""
    check_horizons = staticmethod(_capi.check_horizons)
    SMO_KDYN, SMO_SH23 = _capi.SMO_KDYN, _capi.SMO_SH23

    def Context(self, *a, **k):
        raise AssertionError("a device context was opened")

    MultiContext = Context


_BAD = [([], "empty"), ([3, 0, 2], "member 1"), ([3, -1], "member 1"), ([2, 2.5], "member 1"), ([2.0, 3], "member 0"), ([True, 3], "member 0")]


@pytest.mark.parametrize("seq,msg", _BAD)
def test_kdyn_front_end_refuses_before_any_device_call(monkeypatch, seq, msg):
    monkeypatch.setattr(kdyn, "_capi", _NoDevice())
    dom = kdyn.KDynDomain(16)
    for kw in ({}, {"frozen_U": True}, {"frozen_U": True, "keep_states": False}):
        with pytest.raises(ValueError, match=msg):
            dom.context(1.3, 1e-2, seq, "Final", **kw)
        assert dom._ctx == {}


def test_kdyn_front_end_refuses_contradicting_lengths_and_devices(monkeypatch):
    monkeypatch.setattr(kdyn, "_capi", _NoDevice())
    dom = kdyn.KDynDomain(16)
    with pytest.raises(ValueError, match="batch = 2"):
        dom.context(1.3, 1e-2, (3, 2, 1), "Final", batch=2)
    with pytest.raises(ValueError, match="Rm"):
        dom.context((1.0, 2.0), 1e-2, (3, 2, 1), "Final")
    with pytest.raises(ValueError, match="member 1"):
        dom.context((1.0, -2.0, 3.0), 1e-2, (3, 2, 1), "Final")
    assert dom._ctx == {}
    dom = kdyn.KDynDomain(16, devices=[0, 0])
    with pytest.raises(ValueError, match="multi-device"):
        dom.context(1.3, 1e-2, (3, 2), "Final")
    assert dom._ctx == {}


@pytest.mark.parametrize("seq,msg", _BAD)
def test_sh23_front_end_refuses_before_any_device_call(monkeypatch, seq, msg):
    monkeypatch.setattr(sh23, "_capi", _NoDevice())
    dom = sh23.SH23Domain(64)
    with pytest.raises(ValueError, match=msg):
        dom.context(0.1, seq)
    with pytest.raises(ValueError, match="batch = 3"):
        dom.context(0.1, (5, 2), batch=3)
    assert dom._ctx == {}


def test_a_sequence_is_a_cache_key_of_its_own(monkeypatch):
    made = []

    class Recorder(_NoDevice):
        def Context(self, *a, **k):
            made.append((a, k))

            class Ctx:
                batch = k.get("batch", 1)
                horizons = None

                def set_horizons(self, hz):
                    self.horizons = tuple(hz)

                def close(self):
                    pass
            return Ctx()

    monkeypatch.setattr(kdyn, "_capi", Recorder())
    dom = kdyn.KDynDomain(16)
    c1 = dom.context((0.7, 1.3, 2.9), 1e-2, [4, 1, 3], "Integrated", frozen_U=True)
    assert c1.horizons == (4, 1, 3) and c1.batch == 3
    (a, k), = made
    assert a[4] == 4 and a[5] == (0.7, 1.3, 2.9) and k["batch"] == 3 and k["frozen_u"]       # capacity = the longest horizon
    assert dom.context((0.7, 1.3, 2.9), 1e-2, (4, 1, 3), "Integrated", frozen_U=True) is c1
    c2 = dom.context((0.7, 1.3, 2.9), 1e-2, (4, 2, 3), "Integrated", frozen_U=True)
    assert c2 is not c1 and len(made) == 2
    c3 = dom.context(1.3, 1e-2, np.array([2, 5]), "Final")
    assert c3.horizons == (2, 5) and made[-1][0][4] == 5 and made[-1][1]["batch"] == 2


def _pairwise_min(values):
    return min(abs(a - b) / max(abs(a), abs(b)) for a, b in itertools.combinations(values, 2))


@pytest.mark.parametrize("cost", ["Final", "Integrated"])
def test_kdyn_oracle_J_depends_on_the_horizon(cost):
    from oracle.kdyn import KDynOracle
    (B0, U), = _members(24, [0])
    J = [KDynOracle(16, Rm=1.3, dt=1e-2, N_ITERS=n, Cost_function=cost).forward([B0, U]) for n in (1, 2, 3, 4, 6)]
    print(cost, J, _pairwise_min(J))
    assert _pairwise_min(J) > 1e-2


def test_sh23_oracle_J_depends_on_the_horizon():
    from oracle.sh23 import SH23Oracle
    X = sh23_input(64)
    J = [SH23Oracle(64, dt=0.1, N_ITERS=n).forward([X]) for n in (1, 5, 10, 20)]
    print(J, _pairwise_min(J))
    assert _pairwise_min(J) > 1e-2
