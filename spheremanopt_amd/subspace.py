"""Block (subspace) iteration for the leading seeds of a linear propagator: the k most amplified initial conditions and their growth factors,
i.e. the leading right singular vectors and squared singular values of A in J(x) = <A x, A x>.

A power iteration per member (examples/kdyn_growth_curve.py) finds the optimum alone.  The sub-optimal modes need the members to meet: the
Gram matrix <x_a, y_b> and the recombination out_b = sum_a C[a][b] x_a (smo_gram*, smo_combine*).  This module is host-only linear algebra
on k x k matrices, written against a small backend that owns the vectors:

    backend.gram(X, Y)     -> (k, k) array of <x_a, y_b>
    backend.combine(X, C)  -> the block with members out_b = sum_a C[a][b] x_a
    backend.apply(X)       -> A^T A applied to every member

NumpyBackend keeps the members as the rows of an array (tests, the oracle); ContextBackend keeps them in HBM on a batched frozen-velocity KDyn
context, where apply is one forward and one adjoint solve of the whole batch.
"""
import numpy as np


def orthonormalise(backend, X, passes=2):
    """Cholesky-QR: G = gram(X, X) = R^T R, X <- combine(X, R^-1), `passes` times (the second pass removes what the first one's conditioning
    left).  Returns (X, R) with the input block = X.R, R the accumulated upper-triangular factor.  numpy.linalg.LinAlgError when G is not
    positive definite to working precision: the block is rank-deficient."""
    R_acc = None
    for p in range(1, int(passes) + 1):
        G = np.asarray(backend.gram(X, X), dtype=np.float64)
        G = 0.5 * (G + G.T)
        k = G.shape[0]
        if not np.all(np.isfinite(G)):
            raise np.linalg.LinAlgError("orthonormalise: pass %d: the Gram matrix has non-finite entries" % p)
        try:
            L = np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            raise np.linalg.LinAlgError("orthonormalise: pass %d: the Gram matrix is not positive definite (rank-deficient block)" % p) from None
        # a pivot at rounding level of its diagonal entry is a dependent member that rounding happened to leave positive
        if np.any(np.diag(L) ** 2 <= 4.0 * k * np.finfo(np.float64).eps * np.diag(G)):
            raise np.linalg.LinAlgError("orthonormalise: pass %d: the Gram matrix is not positive definite to working precision "
                                        "(rank-deficient block)" % p)
        R = L.T
        X = backend.combine(X, np.linalg.solve(R, np.eye(k)))
        R_acc = R if R_acc is None else R @ R_acc
    return X, R_acc


def leading_seeds(backend, X0, iters):
    """Subspace iteration with Rayleigh-Ritz on A^T A.  Each sweep: X <- orthonormalise(apply(X)); T = gram(X, apply(X)), symmetrised; eigh;
    X <- combine(X, V).  Returns (Ritz values in descending order, the seeds — orthonormal, seed b belonging to value b —, the history of the
    Ritz values, one row per sweep).  apply is linear, so the next sweep's apply(X) is combine(apply(X), V) of this one: one apply per sweep
    after the first."""
    if int(iters) < 1:
        raise ValueError("leading_seeds: iters = %r (at least one sweep)" % (iters,))
    X, AX, history = X0, backend.apply(X0), []
    for _ in range(int(iters)):
        X, _ = orthonormalise(backend, AX)
        AX = backend.apply(X)
        T = np.asarray(backend.gram(X, AX), dtype=np.float64)
        w, V = np.linalg.eigh(0.5 * (T + T.T))
        w, V = w[::-1].copy(), np.ascontiguousarray(V[:, ::-1])
        X, AX = backend.combine(X, V), backend.combine(AX, V)
        history.append(w)
    return history[-1], X, np.array(history)


class NumpyBackend:
    """Members are the rows of a (k, n) array.  matvec / rmatvec: x -> A x and y -> A^T y on one member; inner(x, y): the inner product A^T is
    taken in (default: the plain dot product)."""

    def __init__(self, matvec, rmatvec, inner=None):
        self.matvec, self.rmatvec = matvec, rmatvec
        self.inner = inner if inner is not None else (lambda x, y: float(np.dot(x, y)))

    def gram(self, X, Y):
        return np.array([[self.inner(x, y) for y in Y] for x in X])

    def combine(self, X, C):
        return np.asarray(C, dtype=np.float64).T @ np.asarray(X, dtype=np.float64)

    def apply(self, X):
        return np.array([self.rmatvec(self.matvec(x)) for x in X])


class ContextBackend:
    """A batched frozen-velocity KDyn context (domain.context(..., batch=k, frozen_U=True), "Final" cost): the block is ONE DeviceVector
    [k][vec_len] that never leaves HBM.  forward returns -<A x_b, A x_b> per member and the adjoint its gradient -2 A^T A x_b, so apply is
    forward_dev, adjoint_dev and the factor -1/2.  U: the given flow — one member's vector (NumPy or DeviceVector of vec_len entries, repeated for
    every member) or the full [k][vec_len] DeviceVector."""

    def __init__(self, ctx, U, adjoint_type="Discrete"):
        from .devvec import DeviceVector
        if not getattr(ctx, "frozen_u", False):
            raise ValueError("ContextBackend: a frozen-velocity context expected (the seeds are fields B0 at a given flow)")
        self.ctx, self.adjoint_type, self._DV = ctx, adjoint_type, DeviceVector
        full = ctx.vec_len * ctx.batch
        if hasattr(U, "ptr") and U.n == full:
            self.U = U
        else:
            u = np.asarray(U.numpy() if hasattr(U, "numpy") else U, dtype=np.float64).reshape(-1)
            if u.size != ctx.vec_len:
                raise ValueError("ContextBackend: U has %d entries, %d (one member) or %d (the batch) expected" % (u.size, ctx.vec_len, full))
            self.U = DeviceVector.from_numpy(np.tile(u, ctx.batch), ctx.cfg.device)

    def block(self, X):
        """(k, vec_len) host array -> the DeviceVector block."""
        return self._DV.from_numpy(np.ascontiguousarray(X, dtype=np.float64).reshape(-1), self.ctx.cfg.device)

    def gram(self, X, Y):
        return self.ctx.gram_dev(X, None if Y is X else Y)

    def combine(self, X, C):
        return self.ctx.combine_dev(C, X)

    def growth(self, X):
        """<A x_b, A x_b> of every member: one forward solve."""
        return -np.atleast_1d(self.ctx.forward_dev([X, self.U]))

    def apply(self, X):
        self.ctx.forward_dev([X, self.U])
        g = self._DV(self.ctx.vec_len * self.ctx.batch, self.ctx.cfg.device)
        self.ctx.adjoint_dev([X, self.U], [g], self.adjoint_type)
        return -0.5 * g
