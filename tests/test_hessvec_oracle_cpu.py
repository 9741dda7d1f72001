"""Pins the NumPy restatement of the SH23 tangent / second-order adjoint sweeps (hessvec_ops.py) against the oracle, on the CPU.

Six checks per case; observed on the five cases: by-product gradient equal to oracle.adjoint bit for bit; |df - <V, grad f>| / |df| <= 1.5e-14;
central differences of the oracle gradient converge to H.V with an error ratio of 100.0 +- 0.05 between eps = 1e-3 and 1e-4; symmetry to
6e-16; scaling by powers of two exact; third Taylor remainder slopes within 0.051 of 3 (worst: Npts 21).
"""
import numpy as np
import pytest

import hessvec_ops as ho

IDS = ["%d-%g-%d" % c for c in ho.CASES]


@pytest.fixture(scope="module", params=ho.CASES, ids=IDS)
def case(request):
    Npts, dt, N = request.param
    o = ho.oracle(Npts, dt, N)
    X, V, W = ho.inputs(Npts)
    df, g, HV = ho.hessvec(o, X, V)
    return {"o": o, "X": X, "V": V, "W": W, "df": df, "g": g, "HV": HV}


def test_by_product_gradient_is_the_oracles(case):
    o = case["o"]
    o.forward([case["X"]])
    assert np.array_equal(case["g"], o.adjoint([case["X"]])[0])


def test_directional_derivative(case):
    o = case["o"]
    d = o.inner(case["V"], case["g"])
    print("df %.16e  <V, grad> %.16e  rel %.2e" % (case["df"], d, abs(case["df"] - d) / abs(case["df"])))
    assert abs(case["df"] - d) <= 1e-12 * abs(case["df"])


def test_central_differences_of_the_gradient_converge_quadratically(case):
    o, X, V, HV = case["o"], case["X"], case["V"], case["HV"]

    def grad(Y):
        o.forward([Y])
        return o.adjoint([Y])[0]
    err = [np.linalg.norm((grad(X + e * V) - grad(X - e * V)) / (2. * e) - HV) for e in (1e-3, 1e-4)]
    print("FD errors", err, "ratio", err[0] / err[1])
    assert 90. <= err[0] / err[1] <= 110.


def test_symmetry(case):
    o, X, V, W = case["o"], case["X"], case["V"], case["W"]
    HW = ho.hessvec(o, X, W)[2]
    a, b = o.inner(W, case["HV"]), o.inner(V, HW)
    print("<W,HV> %.16e  <V,HW> %.16e  rel %.2e" % (a, b, abs(a - b) / abs(a)))
    assert abs(a - b) <= 1e-12 * abs(a)


def test_power_of_two_scaling_is_exact(case):
    o, X, V = case["o"], case["X"], case["V"]
    assert np.array_equal(ho.hessvec(o, X, 8. * V)[2], 8. * case["HV"])
    assert np.array_equal(ho.hessvec(o, X, V / 8.)[2], case["HV"] / 8.)


def test_third_taylor_remainder(case):
    o, X, V = case["o"], case["X"], case["V"]
    f0 = o.forward([X])
    d1, d2 = o.inner(V, case["g"]), o.inner(V, case["HV"])
    eps = 0.1 * 0.5 ** np.arange(5)
    R3 = np.array([abs(o.forward([X + e * V]) - f0 - e * d1 - 0.5 * e * e * d2) for e in eps])
    slopes = np.log(R3[:-1] / R3[1:]) / np.log(2.)
    print("R3", R3, "slopes", slopes)
    assert np.all(np.abs(slopes[-3:] - 3.) <= 0.06)
