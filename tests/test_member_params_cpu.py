"""One parameter value per batch member (smo_create_members: KDYN Rm, SH23 a), host-side checks (no GPU): what the front end refuses before
any device call, and — on the oracle alone — that the values the GPU tests give their members move J by far more than the tolerance, so a
kernel that ignored a member's value cannot pass them."""
import itertools

import numpy as np
import pytest

import parameter_cases as pc
from spheremanopt_amd import _capi, kdyn
from test_kdyn_batch_gpu import _members

RMS = (0.7, 1.3, 2.9)
SH_A = (0.2, -1.7, -0.3)


def _refused(dom, match, *args, **kw):
    with pytest.raises(ValueError, match=match):
        dom.context(*args, **kw)
    assert dom._ctx == {}


def test_empty_sequence_is_refused():
    _refused(kdyn.KDynDomain(16), "empty", [], 1e-2, 3, "Final")


def test_length_contradicting_an_explicit_batch_is_refused():
    _refused(kdyn.KDynDomain(16), "contradicts", RMS, 1e-2, 3, "Final", batch=2)


@pytest.mark.parametrize("bad", [0., -1.3, float("nan"), float("inf")])
def test_values_that_are_not_positive_and_finite_are_refused(bad):
    _refused(kdyn.KDynDomain(16), "member 1", (0.7, bad, 2.9), 1e-2, 3, "Final")


def test_multi_device_domain_is_refused():
    dom = kdyn.KDynDomain(16, devices=[0, 0])
    _refused(dom, "one GPU", RMS, 1e-2, 3, "Final")
    _refused(dom, "one GPU", [1.3], 1e-2, 3, "Final")


def test_capi_context_refuses_a_contradicting_batch_without_loading_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_capi, "lib", no_library)
    with pytest.raises(ValueError, match="contradicts"):
        _capi.Context(_capi.SMO_KDYN, 16, (0., 2 * np.pi), 1e-2, 3, RMS, batch=2)
    with pytest.raises(ValueError, match="contradicts"):
        _capi.Context(_capi.SMO_SH23, 64, pc.SH23_DEFAULT[0], 0.1, 20, np.array(SH_A), batch=4)


def test_signature_of_the_new_export():
    import ctypes as C
    restype, argtypes = _capi.SIGNATURES["smo_create_members"]
    assert restype is C.c_int and argtypes == [C.POINTER(_capi.smo_config), C.POINTER(C.c_double), C.POINTER(C.c_void_p)]


def _pairwise_apart(J, tol=1e-2):
    for a, b in itertools.combinations(J, 2):
        assert abs(a - b) > tol * max(abs(a), abs(b)), J


@pytest.mark.parametrize("cost", ["Final", "Integrated"])
def test_oracle_kdyn_rm_moves_the_cost(cost):
    from oracle.kdyn import KDynOracle
    B, U = _members(24, [0])[0]
    J = [KDynOracle(16, Rm=rm, dt=1e-2, N_ITERS=3, Cost_function=cost).forward([B, U]) for rm in RMS]
    _pairwise_apart(J)
    if cost == "Final":
        assert np.allclose(J, (-0.296, -0.375, -0.440), atol=1e-3), J


def test_oracle_sh23_a_moves_the_cost():
    from oracle.sh23 import SH23Oracle
    X = pc.sh23_input(64)
    J = [SH23Oracle(64, interval=pc.SH23_DEFAULT[0], dt=0.1, N_ITERS=20, a=a).forward([X]) for a in SH_A]
    _pairwise_apart(J)
