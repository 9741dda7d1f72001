"""examples/kdyn_growth_curve.py: power iteration on A^T A for several horizons in lockstep on one frozen-velocity context."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_growth_curve_never_loses_energy():
    """For a frozen flow J is a quadratic form and the example's iteration is power iteration on the symmetric positive semidefinite A^T A:
    its Rayleigh quotient -J cannot decrease beyond rounding, for every horizon."""
    from spheremanopt_amd.examples import kdyn_growth_curve
    hz, F = kdyn_growth_curve.main(["--npts", "8", "--horizons", "3,7,5", "--iters", "3", "--adjoint", "Discrete", "--quiet"])
    assert hz == (3, 7, 5) and F.shape == (3, 3)
    print(F)
    assert np.all(F < 0)
    for b in range(3):
        for k in range(2):
            assert F[k + 1, b] <= F[k, b] + 1e-10 * abs(F[k, b]), (b, k, F[:, b])
    assert len(set(F[0])) == 3                                    # one seed, three horizons: three energies
