"""Subspace iteration for the leading seeds of a frozen flow (spheremanopt_amd/subspace.py) on a batched frozen-velocity KDyn context, against
the same iteration driven by the NumPy oracle; and examples/kdyn_leading_seeds.py."""
import numpy as np
import pytest

from oracle.kdyn import KDynOracle
from spheremanopt_amd import kdyn, subspace

pytestmark = pytest.mark.gpu

NPTS, RM, DT, STEPS, K, SWEEPS = 8, 1., 1e-3, 4, 3, 3


def test_context_backend_agrees_with_the_oracle():
    dom = kdyn.KDynDomain(NPTS)
    n = dom.vec_len
    U = kdyn.synthetic_field(dom.G, 2)
    X0 = np.stack([kdyn.synthetic_field(dom.G, 10 + b) for b in range(K)])
    ctx = dom.context(RM, DT, STEPS, "Final", batch=K, frozen_U=True)
    be = subspace.ContextBackend(ctx, U, "Discrete")
    ritz, X, history = subspace.leading_seeds(be, be.block(X0), SWEEPS)

    # the oracle has no A and A^T of their own: its forward solve keeps the states of x (and returns -<A x, A x>), its adjoint then returns
    # the gradient -2 A^T A x of that x.  matvec = "run the forward solve, hand x on", rmatvec = -1/2 of the adjoint's first component.
    o = KDynOracle(NPTS, Rm=RM, dt=DT, N_ITERS=STEPS, Cost_function="Final")

    def matvec(x):
        o.forward([x, U])
        return x

    ref = subspace.NumpyBackend(matvec, lambda x: -0.5 * o.adjoint([x, U], "Discrete")[0], o.inner)
    ritz_o, X_o, history_o = subspace.leading_seeds(ref, X0, SWEEPS)

    print("device Ritz values per sweep\n", history, "\noracle\n", history_o)
    assert history.shape == history_o.shape == (SWEEPS, K)
    assert np.all(np.abs(history - history_o) <= 1e-6 * history_o.max(axis=1, keepdims=True))
    assert np.all(np.diff(ritz) <= 0)
    growth = be.growth(X)                                                   # -J of a forward call on the returned seeds
    print("growth of the seeds", growth)
    assert np.all(np.abs(growth - ritz) <= 1e-6 * ritz.max())
    orth = np.abs(be.gram(X, X) - np.eye(K)).max()
    print("|gram(X, X) - I| = %.3g" % orth)
    # a cap, not a measurement: two Cholesky-QR passes leave n * k * 2^-53 ~ 2e-12 here; one pass or a wrong scale leaves
    # orders of magnitude more
    assert orth <= 1e-10
    assert X.n == K * n
    dom.drop_contexts()


def test_example_returns_descending_growth_factors_that_never_decrease(monkeypatch):
    from spheremanopt_amd.examples import kdyn_leading_seeds
    made = []
    real = kdyn.KDynDomain.__init__

    def recording(self, *a, **k):
        made.append(self)
        real(self, *a, **k)
    monkeypatch.setattr(kdyn.KDynDomain, "__init__", recording)
    history, seeds = kdyn_leading_seeds.main(["--npts", "8", "--n-iters", "4", "--k", "3", "--iters", "3", "--quiet"])
    print(history)
    assert history.shape == (3, 3) and seeds.n == 3 * 3 * 12 ** 3
    assert np.all(history > 0) and np.all(np.diff(history, axis=1) <= 0)           # descending within every sweep
    for s in range(2):                                                           # the leading value does not decrease from sweep to sweep
        assert history[s + 1, 0] >= history[s, 0], history[:, 0]
    assert made and all(d._ctx == {} and d._transform_ctx is None for d in made)    # no context left behind
