"""KDyn with a frozen velocity (smo_create_frozen_u), the parts that need no GPU: the entry point is declared, exported and bound; the Python
front end refuses what the library would refuse before any device call; and the premise of the whole mode — the G^ recursion of the adjoint
never reads nu or omega x B_f — holds on the oracle."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from spheremanopt_amd import _capi, kdyn


def test_entry_point_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smo.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+smo_create_frozen_u\s*\(([^()]*)\)\s*;", hdr)
    assert m, "include/smo.h does not declare smo_create_frozen_u"
    assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")] == ["cfg", "params", "keep_states", "out"]
    assert "smo_create_frozen_u" in _capi.SIGNATURES and "smo_create_frozen_u" in _capi.EXPORTS
    restype, argtypes = _capi.SIGNATURES["smo_create_frozen_u"]
    assert restype is _capi.C.c_int and len(argtypes) == 4 and argtypes[2] is _capi.C.c_int
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(_capi.lib(), "smo_create_frozen_u")


def test_front_end_refusals_come_before_any_device_call():
    dom = kdyn.KDynDomain(16, devices=[0, 0])
    with pytest.raises(ValueError, match="multi-device"):
        dom.context(1.0, 1e-2, 3, "Final", frozen_U=True)
    assert dom._ctx == {}
    dom = kdyn.KDynDomain(16)
    with pytest.raises(ValueError, match="Integrated"):
        dom.context(1.0, 1e-2, 3, "Integrated", frozen_U=True, keep_states=False)
    assert dom._ctx == {}
    with pytest.raises(ValueError, match="frozen_U"):
        dom.context(1.0, 1e-2, 3, "Final", keep_states=False)
    assert dom._ctx == {}
    with pytest.raises(RuntimeError, match="freeze_velocity"):      # the one-sphere callables without a frozen flow
        kdyn.FWD_Solve_IVP_Lin_B([np.zeros(dom.vec_len)], dom, 1.0, 1e-2, 3, 3, kdyn.GEN_BUFFER(16, dom, 3))


@pytest.mark.parametrize("cost", ["Final", "Integrated"])
@pytest.mark.parametrize("adj", ["Discrete", "Continuous"])
def test_grad_B_never_reads_the_velocity_gradient_history(cost, adj):
    """Two oracle adjoint sweeps that differ only in the B_f handed to the F2 = omega x B_f term: dJ/dB0 must be the same array, bit for bit,
    while dJ/dU changes.  (What the frozen-velocity context relies on when it drops that half.)"""
    from oracle.kdyn import KDynOracle

    class OtherF2(KDynOracle):
        """cross(om, B): the call whose second factor is not the velocity is the F2 term — it gets another B_f."""
        swap = False

        def cross(self, A, B):
            if self.swap and B is not self.Ug:
                B = 3.0 * B[::-1] + 0.25
            return KDynOracle.cross(A, B)

    N, n = 8, 4
    G = 3 * N // 2
    B0, U = kdyn.synthetic_field(G, 1), kdyn.synthetic_field(G, 2)
    o = OtherF2(N, Rm=1.3, dt=1e-2, N_ITERS=n, Cost_function=cost)
    o.forward([B0, U])
    gB, gU = o.adjoint([B0, U], adj)
    o.swap = True
    gB2, gU2 = o.adjoint([B0, U], adj)
    assert np.array_equal(gB, gB2)
    assert not np.array_equal(gU, gU2)                          # the other history did reach nu
