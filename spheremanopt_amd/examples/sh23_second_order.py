"""Is the point the optimiser returned a minimum or a saddle?  Swift-Hohenberg on the MI355X path, second order.

A few iterations of Optimise_On_Multi_Sphere on a small SH23 problem, then the extreme eigenvalues of the Riemannian Hessian of
f = -J on the sphere <X, X> = E_0 at the point it stopped: Lanczos (hessian.extreme_eigs) on hessian.riemannian_hessvec, whose
Euclidean Hessian-vector products are exact (sh23.HESS_Solve_IVP_Lin: one tangent and one second-order adjoint sweep per product).

Run:  python -m spheremanopt_amd.examples.sh23_second_order [--npts 16] [--n-iters 20] [--max-iters 3] [--k 31]
"""
import argparse

import numpy as np

from .. import hessian
from ..sh23 import ADJ_Solve_IVP_Lin, FWD_Solve_IVP_Lin, GEN_BUFFER, Generate_IC, HESS_Solve_IVP_Lin, Inner_Prod
from ..sphere_opt import Optimise_On_Multi_Sphere


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--npts", type=int, default=16)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--n-iters", type=int, default=20, help="time steps of the forward solve")
    ap.add_argument("--max-iters", type=int, default=3, help="optimiser iterations before the Hessian is examined")
    ap.add_argument("--k", type=int, default=31, help="Lanczos steps at most")
    ap.add_argument("--tol", type=float, default=1e-8, help="an eigenvalue above -tol * max|theta| counts as non-negative")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args(argv)
    E_0, dt, N = 0.0725, a.dt, a.n_iters
    domain, X_0 = Generate_IC(E_0, Npts=a.npts)
    args_IP = (domain, None)
    args_f = [domain, dt, N, N, GEN_BUFFER(domain, N), None, "Discrete"]
    RESIDUAL, FUNCT, X_opt = Optimise_On_Multi_Sphere([X_0], [E_0], FWD_Solve_IVP_Lin, ADJ_Solve_IVP_Lin, Inner_Prod, args_f, args_IP,
                                                      max_iters=a.max_iters, alpha_k=np.pi, LS='LS_wolfe', CG=True, verbose=not a.quiet)
    X = X_opt[0]

    def inner(x, y):
        return Inner_Prod(x, y, *args_IP)

    f = FWD_Solve_IVP_Lin([X], *args_f)                       # the stack every product below reads
    grad = ADJ_Solve_IVP_Lin([X], *args_f)[0]

    def hess(V):
        return hessian.riemannian_hessvec(X, E_0, V, grad, lambda W: HESS_Solve_IVP_Lin([X], [W], *args_f)[0], inner)

    v0 = np.random.RandomState(1).standard_normal(X.size)
    theta, y_min, y_max = hessian.extreme_eigs(hess, v0, inner, a.k, project=lambda Z: Z - (inner(X, Z) / E_0) * X)
    scale = float(np.max(np.abs(theta)))
    res = []
    for th, y in ((theta[0], y_min), (theta[-1], y_max)):
        r = hess(y) - th * y
        res.append(inner(r, r) ** 0.5)
    minimum = bool(theta[0] >= -a.tol * scale)
    if not a.quiet:
        print("f = %.12e after %d optimiser iterations; %d Lanczos steps" % (f, len(FUNCT), len(theta)))
        print("Riemannian Hessian of -J: theta_min = %.6e, theta_max = %.6e (residuals %.1e, %.1e)" % (theta[0], theta[-1], res[0], res[1]))
        print("verdict: " + ("every Ritz value >= -%g * max|theta|: a minimum of -J on the sphere" % a.tol if minimum else
                             "a saddle (or not converged yet): -J decreases along y_min, curvature %.6e" % theta[0]))
    return {"X": X, "f": f, "grad": grad, "theta": theta, "y_min": y_min, "y_max": y_max, "residuals": res, "minimum": minimum,
            "descent_direction": None if minimum else y_min, "v0": v0, "domain": domain, "args_f": args_f}


if __name__ == "__main__":
    main()
