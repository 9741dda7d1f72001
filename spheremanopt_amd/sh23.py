"""1-D periodic Swift-Hohenberg 2-3 — the reference's callbacks, backed by the HIP kernels of csrc/sh23.hip.

Same names / positional signatures as Example_Problems/Periodic_Domain(Fourier)/Swift_Hohenberg/FWD_Solve_SH23.py:

    FWD_Solve_IVP_Lin(X_k, domain, dt, N_ITERS, N_SUB_ITERS, X_FWD_DICT, filename=None, Adjoint_type="Discrete")   :409
    ADJ_Solve_IVP_Lin(X_k, domain, dt, N_ITERS, N_SUB_ITERS, X_FWD_DICT, filename=None, Adjoint_type="Discrete")   :598
    Inner_Prod(x, y, domain, rand_arg=None)                                                                        :158
    Generate_IC(E_0, Npts, X)  -> (domain, X_0)                                                                    :174
    GEN_BUFFER(domain, N_SUB_ITERS, Npts)  -> {'A_fwd': handle}                                                    :238

and, beyond the reference (second order; the kernels of csrc/sh23_hessvec.hpp):

    HESS_Solve_IVP_Lin(X_k, V_k, domain, dt, N_ITERS, N_SUB_ITERS, X_FWD_DICT, filename=None, Adjoint_type="Discrete")  -> [H.V]

so the reference's driver lines work unchanged:

    args_IP = (domain, None); args_f = [domain, dt, N_ITERS, N_SUB_ITERS, X_FWD_DICT, None, Adjoint_type]
    Optimise_On_Multi_Sphere([X_0], [E_0], FWD_Solve_IVP_Lin, ADJ_Solve_IVP_Lin, Inner_Prod, args_f, args_IP, ...)

The ``domain`` slot carries a :class:`SH23Domain` (geometry + cache of device contexts) instead of a Dedalus domain;
``X_FWD_DICT['A_fwd']`` is a handle to the HBM-resident snapshot stack instead of a NumPy array.
"""
import numpy as np

from . import _capi
from ._domain import DomainBase, SnapshotStack, attach

A_PARAM = -0.3       # FWD_Solve_SH23.py:309


class SH23Domain(DomainBase):
    """Geometry of the periodic box + owner of the device contexts (one per (dt, N_ITERS, batch))."""
    _DEFAULT = (0.1, 1)

    def __init__(self, Npts=256, X=(0., 12. * np.pi), dealias=2, device=0):
        super().__init__()
        self.Npts, self.interval, self.dealias, self.device = int(Npts), (float(X[0]), float(X[1])), dealias, device
        self.G = int(dealias * Npts)
        self.Nc = (self.Npts - 1) // 2 + 1
        self.hypervolume = self.interval[1] - self.interval[0]

    def grid(self):
        return self.interval[0] + self.hypervolume * np.arange(self.G) / self.G

    def context(self, dt, N_ITERS, batch=1):
        """N_ITERS a sequence: one horizon per member (smo_set_horizons).  The batch is its length (an explicit `batch` must be 1 or agree),
        the context is created with its maximum as capacity and the horizons are set at creation; member b then equals, bit for bit, a
        batch-1 solve of N_ITERS[b] steps.  The tuple is part of the cache key."""
        if np.ndim(N_ITERS) != 0:
            hz = _capi.check_horizons(N_ITERS)
            if int(batch) not in (1, len(hz)):
                raise ValueError("batch = %d contradicts the %d values of N_ITERS (one per member)" % (batch, len(hz)))
            return super().context(float(dt), hz, batch=len(hz))
        return super().context(float(dt), int(N_ITERS), batch=batch)

    def _make_context(self, dt, N_ITERS, batch):
        if isinstance(N_ITERS, tuple):
            ctx = self._make_context(dt, max(N_ITERS), batch)
            try:
                ctx.set_horizons(N_ITERS)
            except Exception:
                ctx.close()
                raise
            return ctx
        return _capi.Context(_capi.SMO_SH23, self.Npts, self.interval, dt, N_ITERS, A_PARAM, batch=batch, device=self.device)


def _band_limited_noise(dom, seed, E_0):
    """Seeded standard-normal noise on the scale-2 grid, truncated to the Nc retained modes, modes with index fraction > 1/2
    removed (the reference's ``filter_field``, FWD_Solve_SH23.py:28-53), scaled to <X,X> = E_0."""
    G, Nc = dom.G, dom.Nc
    noise = np.random.RandomState(seed).standard_normal(G)
    c = np.fft.rfft(noise) / G
    keep = np.zeros(G // 2 + 1, dtype=bool)
    keep[:Nc] = np.linspace(0, 1, Nc, endpoint=False) <= 0.5
    c[~keep] = 0
    x = np.fft.irfft(c, n=G) * G
    return x * np.sqrt(E_0 / np.mean(x * x))


def FWD_Solve_IVP_PREP(X_k, domain, dt=1e-02, N_ITERS=100, N_SUB_ITERS=100):
    """Smooth an initial condition by integrating it N_ITERS+1 steps with the forward solver ON THE DEVICE and return the
    final state on the scale-2 grid (FWD_Solve_SH23.py:334-407; the reference's solver stops at iteration N_ITERS+1)."""
    ctx = domain.context(dt, N_ITERS + 1)
    ctx.forward([X_k[0]])
    c = ctx.snapshot(N_ITERS + 1).view(np.complex128)
    pad = np.zeros(domain.G // 2 + 1, dtype=complex)
    pad[:domain.Nc] = c
    pad[0] = pad[0].real
    return np.fft.irfft(pad, n=domain.G) * domain.G


def Generate_IC(E_0=1.0, Npts=256, X=(0., 12. * np.pi), seed=42, device=0, prep=False):
    """Domain + initial condition with <X,X> = E_0 (FWD_Solve_SH23.py:174-236): seeded noise (seed 42 in the reference),
    filtered, normalised; with ``prep=True`` additionally smoothed by 101 device steps at dt = 0.01 and re-normalised, which
    is the reference's full recipe.  ``prep=False`` is the synthetic-input recipe of SURVEY.md 8d used by the tests/bench."""
    dom = SH23Domain(Npts, X, device=device)
    x = _band_limited_noise(dom, seed, E_0)
    if prep:
        x = FWD_Solve_IVP_PREP([x], dom)
        x = x * np.sqrt(E_0 / np.mean(x * x))
    return dom, x


def Vec_to_Field(domain, X):
    """The reference scatters the flat vector into a Dedalus field on the scale-2 grid (FWD_Solve_SH23.py:130-156).  Here the flat
    vector IS the grid layout the device kernels read: this returns it as the (G,) grid array (a view, no copy, no MPI scatter)."""
    x = np.asarray(X, dtype=np.float64).reshape(-1)
    if x.size != domain.G:
        raise ValueError("vector has %d entries, the scale-2 grid has %d" % (x.size, domain.G))
    return x


def Field_to_Vec(domain, F):
    """Inverse of Vec_to_Field (FWD_Solve_SH23.py:89-128: gather + allgather): the grid array is the flat vector."""
    return np.ascontiguousarray(F, dtype=np.float64).reshape(-1)


def Integrate_Field(domain, F):
    """(1/L) integ F dx of a field given on the scale-2 grid = its grid mean (FWD_Solve_SH23.py:66-87)."""
    return float(np.mean(np.asarray(F, dtype=np.float64)))


def GEN_BUFFER(domain, N_SUB_ITERS, Npts=256):
    """'A_fwd': ``stack[:, i]`` reads the Nc complex coefficients of snapshot i."""
    return {'A_fwd': SnapshotStack((domain.Nc, N_SUB_ITERS + 1), lambda ctx, i: ctx.snapshot(i).view(np.complex128), "FWD_Solve_IVP_Lin")}


def _check_window(N_ITERS, N_SUB_ITERS):
    if N_SUB_ITERS != N_ITERS:
        raise NotImplementedError("windowed checkpointing (N_SUB_ITERS < N_ITERS) is not implemented (nor in the reference)")


def FWD_Solve_IVP_Lin(X_k, domain, dt, N_ITERS, N_SUB_ITERS, X_FWD_DICT, filename=None, Adjoint_type="Discrete"):
    """-J(X) with J = dt * sum_{n=0}^{N} (1/L) int u_n^2 dx; fills the device snapshot stack."""
    _check_window(N_ITERS, N_SUB_ITERS)
    ctx = domain.context(dt, N_ITERS)
    J = ctx.forward_any([X_k[0]])                          # NumPy vector or devvec.DeviceVector
    attach(X_FWD_DICT, ctx)
    if getattr(domain, "write_products", False):           # scalar_data/ and CheckPoints/ like the reference's file handlers
        from . import products
        products.write_sh23(domain, ctx, dt, N_ITERS)
    return J


def File_Manips(k):
    """The reference's optimiser callback (FWD_Solve_SH23.py:731-746): keep this iteration's scalar_data / CheckPoints files."""
    from . import products
    products.File_Manips(k)


def ADJ_Solve_IVP_Lin(X_k, domain, dt, N_ITERS, N_SUB_ITERS, X_FWD_DICT, filename=None, Adjoint_type="Discrete"):
    """[dJ/dX] on the scale-2 grid; valid right after FWD_Solve_IVP_Lin at the same X_k (it replays that stack)."""
    _check_window(N_ITERS, N_SUB_ITERS)
    ctx = domain.context(dt, N_ITERS)
    return ctx.adjoint_any([X_k[0]], Adjoint_type)


def HESS_Solve_IVP_Lin(X_k, V_k, domain, dt, N_ITERS, N_SUB_ITERS, X_FWD_DICT, filename=None, Adjoint_type="Discrete"):
    """[H.V] on the scale-2 grid, H the Hessian of what FWD_Solve_IVP_Lin returns: the exact derivative of the Discrete gradient in the
    direction V_k[0].  Valid right after FWD_Solve_IVP_Lin at the same X_k (it reads that stack), for any number of directions; the
    gradient callback stays valid before and after."""
    if Adjoint_type != "Discrete":
        raise ValueError("HESS_Solve_IVP_Lin: Adjoint_type=%r — only the Discrete adjoint is the gradient of the discrete cost and has a "
                         "Hessian; differentiating the Continuous adjoint would give an operator that is not symmetric" % (Adjoint_type,))
    _check_window(N_ITERS, N_SUB_ITERS)
    ctx = domain.context(dt, N_ITERS)
    return ctx.hessvec_any([V_k[0]])[0]


def Inner_Prod(x, y, domain, rand_arg=None):
    """(1/L) int x y dx = mean over the scale-2 grid."""
    return domain.any_context().inner_any(x, y)
