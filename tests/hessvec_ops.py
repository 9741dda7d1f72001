"""NumPy restatement of the SH23 tangent and second-order adjoint sweeps (the yardstick of the Hessian-vector tests), built on the oracle's
to_coeff / to_grid / A, in the oracle's notation:

    forward   u^_0 = F X,  u_n = F^-1 u^_n,  u^_{n+1} = (u^_n / dt + F[N(u_n)]) / A,   f = -dt sum_{n=0..N} mean(u_n^2)
    tangent   d^_0 = F V;  for n = 0..N:  d_n = F^-1 d^_n,  df += -2 dt mean(u_n d_n),  d^_{n+1} = (d^_n / dt + F[N'(u_n) d_n]) / A
    soa       q^ = -2 u^_N / A,  r^ = -2 d^_N / A;  for idx = N-1..0:  q^ <- (q^ / dt + F[N'(u) q - 2 u]) / A,
              r^ <- (r^ / dt + F[N'(u) r + N''(u) d q - 2 d]) / A;   grad f = F^-1[dt A q^],  H V = F^-1[dt A r^]

with N(u) = 1.8 u^2 - u^3, N'(u) = 3.6 u - 3 u^2, N''(u) = 3.6 - 6 u.  tests/test_hessvec_oracle_cpu.py pins it (gradient equal to the oracle's
bit for bit, directional derivative, central differences of the oracle gradient, symmetry, exact scaling, third Taylor remainder).
"""
import numpy as np

from oracle.sh23 import SH23Oracle, synthetic_ic

E0 = 0.0725
SEED_X, SEED_V, SEED_W = 42, 7, 9
# (Npts, dt, N) of the CPU pin
CASES = [(16, 0.1, 3), (32, 0.05, 17), (64, 0.1, 40), (21, 0.1, 12), (256, 0.1, 500)]


def inputs(Npts):
    """X, V, W on the scale-2 grid of Npts modes."""
    G = 2 * Npts
    return synthetic_ic(G, SEED_X, E0), synthetic_ic(G, SEED_V, E0), synthetic_ic(G, SEED_W, E0)


def oracle(Npts, dt, N, a=-0.3):
    return SH23Oracle(Npts, dt=dt, N_ITERS=N, a=a)


def tangent(o, V):
    """(df, tangent stack [Nc, N+1]); needs o.forward at X first."""
    dt, N, S = o.dt, o.N_ITERS, o.stack
    D = np.zeros_like(S)
    dh = o.to_coeff(np.asarray(V, dtype=float))
    df = 0.
    for n in range(N + 1):
        D[:, n] = dh
        u, d = o.to_grid(S[:, n]), o.to_grid(dh)
        df += -2. * dt * np.mean(u * d)
        dh = (dh / dt + o.to_coeff((3.6 * u - 3. * u * u) * d)) / o.A
    return df, D


def soa(o, D):
    """(grad f, H V) from the forward stack o.stack and the tangent stack D."""
    dt, N, S = o.dt, o.N_ITERS, o.stack
    qh = -2. * S[:, N] / o.A
    rh = -2. * D[:, N] / o.A
    for idx in range(N - 1, -1, -1):
        u, d, q, r = o.to_grid(S[:, idx]), o.to_grid(D[:, idx]), o.to_grid(qh), o.to_grid(rh)
        n1 = 3.6 * u - 3. * u * u
        qh = (qh / dt + o.to_coeff(n1 * q - 2. * u)) / o.A
        rh = (rh / dt + o.to_coeff(n1 * r + (3.6 - 6. * u) * d * q - 2. * d)) / o.A
    return o.to_grid(dt * o.A * qh), o.to_grid(dt * o.A * rh)


def hessvec(o, X, V):
    """(df, grad f, H V) at X in the direction V; runs the oracle's forward solve at X (o.stack is then X's)."""
    o.forward([X])
    df, D = tangent(o, V)
    g, HV = soa(o, D)
    return df, g, HV


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))
