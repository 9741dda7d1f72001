"""The device's Chebyshev transforms of SHB23 and Poiseuille Discrete, column by column against the closed-form longdouble matrices of
transform_ops.py: every length class of the SHB23 DCT pair (the nine instantiations, every run-time plan class, SMO_SHB_ANY=1) and every
tile-remainder class of the Poiseuille products (pois_gemm), on needles, one seeded white input, the constant 1 and the alternating +-1.
The tolerances are 8 x what the oracle itself reaches against the same matrices (test_transforms_exact_cpu.py)."""
import numpy as np
import pytest

import transform_ops as to
from transform_ops import TOL_ULP

from spheremanopt_amd import poiseuille as pz, shb23

pytestmark = pytest.mark.gpu


def _judge(family, size, worst):
    for kind in ("needle", "dense"):
        d, where = worst[kind]
        print("TRANSFORM-DEFECT %s %s %s %.3f ulp at %s (tolerance %d)" % (family, size, kind, d, where, TOL_ULP[family, kind]))
    for kind in ("needle", "dense"):
        d, where = worst[kind]
        assert d <= TOL_ULP[family, kind], (family, size, kind, d, where)


def _shb_case(N):
    dom = shb23.SHBDomain(N)
    try:
        fns = [lambda x, f=f: f(x, dom) for f in (shb23.transform, shb23.transformInverse, shb23.transformAdjoint, shb23.transformInverseAdjoint)]
        return to.shb_worst(N, fns)
    finally:
        dom.drop_contexts()


@pytest.mark.parametrize("N", to.SHB_LENGTHS)
def test_shb23_transforms_column_by_column(N):
    _judge("shb23", N, _shb_case(N))


@pytest.mark.parametrize("N", to.SHB_ANY_FORCED)
def test_shb23_transforms_column_by_column_through_the_run_time_plan(N, monkeypatch):
    monkeypatch.setenv("SMO_SHB_ANY", "1")
    _judge("shb23", "%d (any-N form)" % N, _shb_case(N))


@pytest.mark.parametrize("Nx,Nz", to.POIS_SHAPES)
def test_poiseuille_transforms_column_by_column(Nx, Nz):
    dom = pz.PoiseuilleDomain(Nx, Nz)
    try:
        assert dom.a == Nx // 2
        fns = [lambda x, f=f: np.array(f(x, dom)) for f in (pz.transform, pz.transformInverse, pz.transformAdjoint, pz.transformInverseAdjoint)]
        worst = to.pois_worst(Nx, Nz, fns)
    finally:
        dom.drop_contexts()
    _judge("pois", "%d x %d" % (Nx, Nz), worst)
