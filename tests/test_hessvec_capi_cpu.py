"""smo_hessvec / smo_hessvec_dev: exported, bound, and a NULL context is an argument error before any device is touched."""
import ctypes as C
import os

import pytest

from spheremanopt_amd import _capi


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


@pytest.mark.parametrize("name", ["smo_hessvec", "smo_hessvec_dev"])
def test_exported_and_bound(L, name):
    assert name in _capi.EXPORTS and hasattr(L, name)
    restype, argtypes = _capi.SIGNATURES[name]
    assert restype is C.c_int and len(argtypes) == 4
    assert getattr(L, name).argtypes == argtypes


@pytest.mark.parametrize("name", ["smo_hessvec", "smo_hessvec_dev"])
def test_null_context_is_an_argument_error(L, name):
    v = (C.c_double * 8)()
    ptrs = _capi._ptr_array([C.addressof(v)])
    assert getattr(L, name)(None, ptrs, ptrs, None) == 1                       # SMO_ERR_ARG
    assert b"null context" in L.smo_last_error()
    assert getattr(L, name)(None, None, None, None) == 1


def test_python_surface():
    from spheremanopt_amd import sh23
    for m in ("hessvec", "hessvec_dev", "hessvec_any"):
        assert callable(getattr(_capi.Context, m))
    with pytest.raises(ValueError, match="Discrete"):
        sh23.HESS_Solve_IVP_Lin([None], [None], None, 0.1, 4, 4, {}, None, "Continuous")
