"""Optimal seed field of a GIVEN flow (the textbook kinematic-dynamo question): the reference's Npts = 24 set-up
(FWD_Solve_KDyn.py:1025-1067) with the velocity frozen, one sphere <B0,B0> = M_0:

    Generate_IC -> domain.freeze_velocity(U) -> GEN_BUFFER -> Optimise_On_Multi_Sphere([B0], [M_0], FWD_..._B, ADJ_..._B, Inner_Prod_3, ...)

The context behind the two callables computes dJ/dB0 alone (smo_create_frozen_u): no omega x B_f half in the adjoint x pass, no grid-side
stack, and with --no-states no snapshot stack either.  The vectors stay in HBM (devvec.DeviceVector).

Run:  python -m spheremanopt_amd.examples.kdyn_seed_field [--npts 24] [--dt 5e-4] [--steps N] [--max-iters 5] [--no-states]
"""
import argparse

from ..devvec import to_device
from ..kdyn import ADJ_Solve_IVP_Lin_B, FWD_Solve_IVP_Lin_B, GEN_BUFFER, Generate_IC, Inner_Prod_3
from ..sphere_opt import Optimise_On_Multi_Sphere


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--npts", type=int, default=24)
    ap.add_argument("--rm", type=float, default=1.0)
    ap.add_argument("--dt", type=float, default=5e-4)
    ap.add_argument("--steps", type=int, default=None, help="N_ITERS (default int(Rm/dt))")
    ap.add_argument("--max-iters", type=int, default=5)
    ap.add_argument("--no-states", action="store_true", help="keep no snapshot stack (keep_states = 0; the Final cost reads B_N alone)")
    ap.add_argument("--quiet", action="store_true")
    a = ap.parse_args(argv)

    Rm, dt, Npts = a.rm, a.dt, a.npts
    N_ITERS = a.steps or int(Rm / dt)
    M_0 = 1.0
    domain, Bx0, Ux = Generate_IC(Npts, (0., 2. * 3.141592653589793), M_0, True, reference_recipe=True, Rm=Rm, dt=dt)
    X_0 = to_device([Bx0], domain.device)
    domain.freeze_velocity(to_device([Ux], domain.device)[0], keep_states=not a.no_states)
    X_FWD_DICT = GEN_BUFFER(Npts, domain, N_ITERS)
    args_f = [domain, Rm, dt, N_ITERS, N_ITERS, X_FWD_DICT, "Final", "Discrete"]
    RESIDUAL, FUNCT, X_opt = Optimise_On_Multi_Sphere(X_0, [M_0], FWD_Solve_IVP_Lin_B, ADJ_Solve_IVP_Lin_B, Inner_Prod_3, args_f,
                                                      (domain, None), max_iters=a.max_iters, alpha_k=100., LS='LS_wolfe', CG=True,
                                                      verbose=not a.quiet)
    return RESIDUAL, FUNCT, X_opt


if __name__ == "__main__":
    R, F, _ = main()
    print("J_k (final magnetic energy) per iteration:", F)
