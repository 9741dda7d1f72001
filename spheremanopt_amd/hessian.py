"""Second-order tools for optimisation on a sphere <X, X> = M, host side.

Everything here is generic over a Hessian-vector callback ``hv`` and an inner product ``inner``: vectors may be NumPy arrays or anything
with ``+``, ``-`` and scalar ``*`` (``devvec.DeviceVector``), and nothing below touches the library — the module imports without it.
``sh23.HESS_Solve_IVP_Lin`` provides ``hv`` for the Swift-Hohenberg problem (``examples/sh23_second_order.py`` puts the pieces together).

    riemannian_hessvec   Hessian of f restricted to the sphere, applied to a vector
    extreme_eigs         Lanczos with full reorthogonalisation: Ritz values and the two extreme Ritz vectors of a symmetric operator
    taylor_table_2       the Taylor table of test_grad.taylor_table with a third remainder row
"""
import numpy as np

__all__ = ["riemannian_hessvec", "extreme_eigs", "taylor_table_2"]


def _project(X, M, Z, inner, args_IP):
    """P_X(Z) = Z - (<X, Z> / M) X: the tangent part of Z at X."""
    return Z - (inner(X, Z, *args_IP) / M) * X


def riemannian_hessvec(X, M, V, grad, hv, inner, args_IP=()):
    """Hess f(X)[V] on the sphere <X, X> = M:   P_X(hv(P_X V)) - (<X, grad> / M) P_X V.

    ``grad`` is the Euclidean gradient at X (a vector), ``hv(W)`` the Euclidean Hessian at X applied to W.  The second term is the
    curvature of the sphere: at a constrained critical point grad = (<X, grad> / M) X, and the multiplier shifts the spectrum."""
    PV = _project(X, M, V, inner, args_IP)
    return _project(X, M, hv(PV), inner, args_IP) - (inner(X, grad, *args_IP) / M) * PV


def extreme_eigs(op, v0, inner, k, project=None, tol=1e-12):
    """At most ``k`` Lanczos steps on the operator ``op`` (symmetric in ``inner``) from the start vector ``v0``.

    Every new direction is orthogonalised against ALL earlier ones, twice, in the given inner product, so the Ritz values carry no
    ghost copies.  ``project`` (optional) is applied to v0 and to every op result: the operator then lives on that subspace (the tangent
    space of a sphere).  The iteration stops early when the Krylov space is exhausted: what is left of the new direction is at most
    ``tol`` times the largest entry of the tridiagonal matrix so far.

    Returns ``(theta, y_min, y_max)``: the Ritz values in ascending order (their number is the number of steps taken) and the unit Ritz
    vectors of the smallest and the largest one."""
    if k < 1:
        raise ValueError("extreme_eigs: k = %d (at least one step)" % k)
    v = project(v0) if project is not None else v0
    nrm = float(inner(v, v)) ** 0.5
    if not nrm > 0.:
        raise ValueError("extreme_eigs: the start vector vanishes (after the projection)")
    Q = [(1. / nrm) * v]
    alpha, beta = [], []
    for j in range(k):
        w = op(Q[j])
        if project is not None:
            w = project(w)
        alpha.append(float(inner(Q[j], w)))
        for _ in range(2):
            for q in Q:
                w = w - float(inner(q, w)) * q
        b = max(float(inner(w, w)), 0.) ** 0.5
        scale = max(max(abs(a) for a in alpha), max(beta, default=0.))
        if j == k - 1 or b <= tol * scale:
            break
        beta.append(b)
        Q.append((1. / b) * w)
    m = len(alpha)
    T = np.diag(alpha) + np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
    theta, S = np.linalg.eigh(T)

    def ritz(col):
        y = float(S[0, col]) * Q[0]
        for i in range(1, m):
            y = y + float(S[i, col]) * Q[i]
        return y
    return theta, ritz(0), ritz(m - 1)


def taylor_table_2(X, dX, f, grad, hv, inner, args_f=(), args_IP=(), epsilon=1e-04, levels=5):
    """The Taylor table of ``test_grad.taylor_table`` with a third remainder:

        R1(eps) = |f(X + eps dX) - f(X)|                                                     -> O(eps)
        R2(eps) = |f(X + eps dX) - f(X) - eps <dX, grad>|                                    -> O(eps^2)
        R3(eps) = |f(X + eps dX) - f(X) - eps <dX, grad> - eps^2 / 2 <dX, hv(dX)>|           -> O(eps^3)

    for ``levels`` values of eps, each half the one before.  Callbacks on plain vectors: ``f(X, *args_f)``, ``grad(X, *args_f)`` and
    ``hv(X, dX, *args_f)`` are called in this order at X (callbacks that replay a forward solve see it first), then f alone at the
    displaced points; ``inner(x, y, *args_IP)``.

    Returns a (7, levels) array: rows eps, R1, R2, R3 and the log-slopes of R1, R2, R3 between consecutive levels (the last slope
    entry of each row stays 0; a remainder that is exactly zero gives a slope of nan)."""
    f0 = f(X, *args_f)
    d1 = inner(dX, grad(X, *args_f), *args_IP)
    d2 = inner(dX, hv(X, dX, *args_f), *args_IP)
    AA = np.zeros((7, levels))
    for level in range(levels):
        df = f(X + epsilon * dX, *args_f) - f0
        AA[0, level] = epsilon
        AA[1, level] = abs(df)
        AA[2, level] = abs(df - epsilon * d1)
        AA[3, level] = abs(df - epsilon * d1 - 0.5 * epsilon * epsilon * d2)
        epsilon = 0.5 * epsilon
    with np.errstate(divide="ignore", invalid="ignore"):
        for row in (1, 2, 3):
            AA[row + 3, :-1] = np.log(AA[row, :-1] / AA[row, 1:]) / np.log(AA[0, :-1] / AA[0, 1:])
    return AA
