"""Exact symmetries of the discrete problems, as operations on the flat vectors the callbacks take and return (shared by
test_symmetry_oracle_cpu.py, which pins them on the oracle, and test_symmetry_gpu.py, which demands them of the kernels).

KDyn   [3][G][G][G], z fastest: periodic translation along an axis; cyclic relabelling of the axes (x, y, z) -> (y, z, x) of the
       coordinates AND the components; J is a quadratic form in B0 (so gB is linear in B0, gU quadratic).
SH23   [G]: translation, reflection x -> -x.
Pois   [2][Gx][Gz]: translation along x.
The other transposition of the KDyn axes (an orientation flip) and a half-turn of the Poiseuille channel are NOT symmetries of the
discrete schemes and are not used.
"""
import numpy as np


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


# ---- KDyn ----------------------------------------------------------------------------------------------------------------------------
def kd_roll(v, G, shifts):
    """Translate by `shifts` = (sx, sy, sz) grid points."""
    return np.roll(np.asarray(v).reshape(3, G, G, G), shifts, axis=(1, 2, 3)).reshape(-1)


def kd_perm(v, G):
    """P: component c of the result is component c - 1 of v, with the coordinates relabelled the same way."""
    return np.ascontiguousarray(np.roll(np.asarray(v).reshape(3, G, G, G), 1, axis=0).transpose(0, 3, 1, 2)).reshape(-1)


def kd_dirty_fields(G, synthetic_field):
    """The dirty inputs of test_kdyn_gpu._fields: not solenoidal, non-zero mean, full spectrum."""
    B, U = synthetic_field(G, 1), synthetic_field(G, 2)
    B = B + 0.2 * np.random.RandomState(9).standard_normal(B.size) + 0.05
    U = U + 0.2 * np.random.RandomState(10).standard_normal(U.size)
    return B, U


def kd_cheap_field(G, seed, mean=0.05):
    """A full-spectrum field without host FFTs: per component a[x] + b[y] + c[z] + p[x] q[y] r[z] of seeded 1-D standard-normal
    vectors, plus a non-zero mean."""
    rs = np.random.RandomState(seed)
    out = np.empty((3, G, G, G))
    for comp in range(3):
        a, b, c, p, q, r = rs.standard_normal((6, G))
        np.multiply(p[:, None, None] * q[None, :, None], r[None, None, :], out=out[comp])
        out[comp] += a[:, None, None]
        out[comp] += b[None, :, None]
        out[comp] += c[None, None, :] + mean
    return out.reshape(-1)


# ---- SH23 ----------------------------------------------------------------------------------------------------------------------------
def sh_roll(x, s):
    return np.roll(np.asarray(x), s)


def sh_reflect(x):
    return np.roll(np.asarray(x)[::-1], 1)


# ---- Poiseuille ----------------------------------------------------------------------------------------------------------------------
def pz_roll(X, gshape, s):
    return np.roll(np.asarray(X).reshape(2, gshape[0], gshape[1]), s, axis=1).reshape(-1)
