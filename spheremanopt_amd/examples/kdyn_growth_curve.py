"""Growth curve of a GIVEN flow: the largest final magnetic energy <B_T,B_T> a seed field of unit energy can reach, as a function of the
horizon T — the set-up of kdyn_seed_field (the reference's Npts = 24 recipe, velocity frozen) with H horizons on ONE frozen-velocity context
whose members each run a horizon of their own (smo_set_horizons: ``domain.context(..., N_ITERS=(N_0, ..., N_{H-1}), frozen_U=True)``).

For a frozen flow the forward map B0 -> B_N is linear, B_N = A B0, so J = <A B0, A B0> is a quadratic form and -grad J = 2 A^T A B0: the
iteration  B0_b <- -grad J_b, rescaled to the sphere <B0_b,B0_b> = 1,  is power iteration on A_b^T A_b.  It runs for all horizons in
lockstep — one forward call and one adjoint call per iteration, whatever H — and its Rayleigh quotient, the energy itself, cannot decrease.
The vectors stay in HBM (devvec.DeviceVector, [H][3 G^3]); every member starts from the same seed.

Run:  python -m spheremanopt_amd.examples.kdyn_growth_curve [--npts 24] [--dt 5e-4] [--horizons 100,200,400] [--iters 5] [--adjoint Discrete]
"""
import argparse

import numpy as np

from .. import _capi
from ..devvec import DeviceVector
from ..kdyn import Generate_IC


def _rescale(ctx, src, dst, factors):
    """dst_b = factors[b] * src_b for every member b (one smo_vec_axpby per member on its slice; dst may be src)."""
    L = ctx.vec_len
    for b, s in enumerate(factors):
        _capi._check(_capi.lib().smo_vec_axpby(src.device, L, float(s), src.ptr + 8 * b * L, 0.0, None, dst.ptr + 8 * b * L))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--npts", type=int, default=24)
    ap.add_argument("--rm", type=float, default=1.0)
    ap.add_argument("--dt", type=float, default=5e-4)
    ap.add_argument("--horizons", default="100,200,400", help="N_ITERS of every member, comma-separated")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--adjoint", default="Discrete", choices=["Discrete", "Continuous"])
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args(argv)

    hz = tuple(int(v) for v in a.horizons.split(","))
    H = len(hz)
    domain, Bx0, Ux = Generate_IC(a.npts, (0., 2. * np.pi), 1.0, True, reference_recipe=True, Rm=a.rm, dt=a.dt)
    ctx = domain.context(a.rm, a.dt, hz, "Final", frozen_U=True, keep_states=False)
    X = [DeviceVector.from_numpy(np.tile(Bx0, H), domain.device), DeviceVector.from_numpy(np.tile(Ux, H), domain.device)]
    g = [DeviceVector(H * ctx.vec_len, domain.device)]
    F = []
    for k in range(a.iters):
        F.append(np.atleast_1d(ctx.forward_dev(X)).copy())       # -<B_N,B_N> per horizon (the value the optimisers minimise)
        if not a.quiet:
            print("iteration %d: -J per horizon %s = %s" % (k, hz, " ".join("%.12e" % -f for f in F[-1])))
        if k + 1 == a.iters:
            break
        ctx.adjoint_dev(X, g, a.adjoint)
        nrm = np.atleast_1d(ctx.inner_dev(g[0], g[0]))
        if not np.all(nrm > 0):
            break                                                  # a seed the flow annihilates: nothing to iterate on
        _rescale(ctx, g[0], X[0], -1. / np.sqrt(nrm))              # B0_b <- -grad J_b / |grad J_b|
    domain.drop_contexts()
    return hz, np.array(F)


if __name__ == "__main__":
    main()
