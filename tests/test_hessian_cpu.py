"""spheremanopt_amd/hessian.py on a known answer: f(x) = x.A.x / 2 with a seeded symmetric 12 x 12 A, the Euclidean dot product, the unit
sphere.  At an eigenvector x_i the Riemannian Hessian has the eigenvectors x_j, j != i, with the eigenvalues lambda_j - lambda_i."""
import os
import subprocess
import sys

import numpy as np
import pytest

from spheremanopt_amd import hessian

N = 12


@pytest.fixture(scope="module")
def quad():
    B = np.random.RandomState(5).standard_normal((N, N))
    A = 0.5 * (B + B.T)
    lam, Xe = np.linalg.eigh(A)
    return A, lam, Xe


def _riem(A, x):
    return lambda V: hessian.riemannian_hessvec(x, 1., V, A @ x, lambda W: A @ W, np.dot)


@pytest.mark.parametrize("i", [0, 5, N - 1])
def test_riemannian_hessvec_at_an_eigenvector(quad, i):
    A, lam, Xe = quad
    op = _riem(A, Xe[:, i])
    for j in range(N):
        want = (lam[j] - lam[i]) * Xe[:, j] if j != i else np.zeros(N)       # x_i itself is normal to the sphere
        assert np.max(np.abs(op(Xe[:, j]) - want)) <= 1e-12
    V = np.random.RandomState(6).standard_normal(N)                          # a direction with a normal part: only its tangent part counts
    PV = V - np.dot(Xe[:, i], V) * Xe[:, i]
    assert np.max(np.abs(op(V) - op(PV))) <= 1e-12


@pytest.mark.parametrize("i", [0, 5, N - 1])
def test_extreme_eigs_finds_the_extreme_gaps(quad, i):
    A, lam, Xe = quad
    x = Xe[:, i]
    op = _riem(A, x)
    gaps = np.delete(lam - lam[i], i)
    theta, ymin, ymax = hessian.extreme_eigs(op, np.random.RandomState(7).standard_normal(N), np.dot, N - 1, project=lambda Z: Z - np.dot(x, Z) * x)
    assert len(theta) == N - 1 and np.all(np.diff(theta) >= 0)
    assert abs(theta[0] - gaps.min()) <= 1e-10 and abs(theta[-1] - gaps.max()) <= 1e-10
    for th, y in ((theta[0], ymin), (theta[-1], ymax)):
        assert abs(np.dot(y, y) - 1.) <= 1e-12 and abs(np.dot(x, y)) <= 1e-12
        assert np.linalg.norm(op(y) - th * y) <= 1e-10


def test_extreme_eigs_stops_on_an_invariant_subspace(quad):
    A, lam, Xe = quad
    calls = []

    def op(V):
        calls.append(1)
        return A @ V
    v0 = Xe[:, 1] + 2. * Xe[:, 4] - 0.5 * Xe[:, 9]
    theta, ymin, ymax = hessian.extreme_eigs(op, v0, np.dot, 11)
    assert len(theta) == 3 and len(calls) == 3
    assert np.max(np.abs(theta - lam[[1, 4, 9]])) <= 1e-12
    assert min(np.linalg.norm(ymin - Xe[:, 1]), np.linalg.norm(ymin + Xe[:, 1])) <= 1e-10
    assert min(np.linalg.norm(ymax - Xe[:, 9]), np.linalg.norm(ymax + Xe[:, 9])) <= 1e-10
    with pytest.raises(ValueError):
        hessian.extreme_eigs(op, np.zeros(N), np.dot, 3)
    with pytest.raises(ValueError):
        hessian.extreme_eigs(op, v0, np.dot, 0)


def test_taylor_table_2(quad):
    A, _, _ = quad
    rs = np.random.RandomState(8)
    c, x, dx = rs.standard_normal(N), rs.standard_normal(N), rs.standard_normal(N)
    # a cubic: the third remainder is exactly eps^3 |sum c dx^3|
    AA = hessian.taylor_table_2(x, dx, lambda y: 0.5 * y @ A @ y + np.sum(c * y ** 3), lambda y: A @ y + 3. * c * y ** 2,
                                lambda y, v: A @ v + 6. * c * y * v, np.dot, epsilon=0.1)
    assert AA.shape == (7, 5) and np.allclose(AA[0], 0.1 * 0.5 ** np.arange(5), rtol=0, atol=0)
    assert np.all(np.abs(AA[6, :4] - 3.) <= 1e-6) and AA[6, 4] == 0.
    e, d1, d2, d3 = AA[0], dx @ (A @ x + 3. * c * x ** 2), dx @ (A @ dx + 6. * c * x * dx), np.sum(c * dx ** 3)
    assert np.allclose(AA[3], e ** 3 * abs(d3), rtol=1e-6)
    assert np.allclose(AA[2], np.abs(0.5 * e ** 2 * d2 + e ** 3 * d3), rtol=1e-9)
    assert np.allclose(AA[1], np.abs(e * d1 + 0.5 * e ** 2 * d2 + e ** 3 * d3), rtol=1e-9)
    assert np.allclose(AA[4:6, :4], np.log2(AA[1:3, :4] / AA[1:3, 1:]), rtol=1e-12) and np.all(AA[4:6, 4] == 0.)
    # a quadratic with small-integer data: every term is exact in binary, the third remainder vanishes identically
    Ai = np.round(4. * A)
    xi, di = np.round(4. * x), np.round(4. * dx)
    AA = hessian.taylor_table_2(xi, di, lambda y: 0.5 * y @ Ai @ y, lambda y: Ai @ y, lambda y, v: Ai @ v, np.dot, epsilon=0.5)
    assert np.all(AA[3] == 0.) and np.all(AA[2] > 0.)
    # the callbacks' extra arguments are passed through
    AA2 = hessian.taylor_table_2(xi, di, lambda y, M: 0.5 * y @ M @ y, lambda y, M: M @ y, lambda y, v, M: M @ v,
                                 lambda a, b, s: s * np.dot(a, b), args_f=(Ai,), args_IP=(1.,), epsilon=0.5, levels=3)
    assert AA2.shape == (7, 3) and np.array_equal(AA2[:4], AA[:4, :3])


def test_hessian_imports_without_the_library():
    code = ("import sys, spheremanopt_amd.hessian as h; bad = [m for m in sys.modules if m.split('.')[0] in ('torch', 'oracle') or "
            "m == 'spheremanopt_amd._capi']; assert not bad, bad; import ctypes; print(len(h.__all__))")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == 3
