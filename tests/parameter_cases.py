"""Physical parameters off the values of the reference scripts (shared by test_parameters_oracle_cpu.py, which shows on the oracle that each
of them moves the answer by far more than the tolerance, and test_parameters_gpu.py, which demands the oracle's answer of the kernels).

Every other test runs Poiseuille at Re = 500, Ri = 0.05, Prandtl = 1, Lx = 4 pi, SH23 at a = -0.3 on (0, 12 pi) and SHB23 at a = -0.1 on
(-20, 20): with Prandtl = 1 a Re where Pe = Re Pr belongs is invisible, and at Ri = 0.05 over six small steps the buoyancy coupling moves
the gradients by less than the tolerance.  The sets below are chosen so that no two parameters coincide and none is 1.
"""
import numpy as np

from symmetry_ops import rel  # noqa: F401  (|a - b| / |b|, shared with the symmetry tests)

# ---- Poiseuille ------------------------------------------------------------------------------------------------------------------------
POIS_P = dict(Re=200., Ri=2.0, Prandtl=0.5, Lx=7.0)
POIS_DEFAULT = dict(Re=500., Ri=0.05, Prandtl=1., Lx=4. * np.pi)
POIS_DT, POIS_N, POIS_DELTA = 2e-2, 10, 0.3
POIS_DISCRETE_SIZES = [(24, 24), (48, 36)]
POIS_CNTS_SIZES = [(16, 16), (32, 24)]
POIS_BATCH_SEEDS = (42, 7, 3)
POIS_PE_PAIRS = [(500., 2.), (1000., 1.), (250., 4.)]       # Re Pr = 1000 each; the products and Pe / Re are exact in binary
POIS_PE_OTHER = (500., 1.)
_POIS_X = {}


def pois_oracle(Nx, Nz, s, continuous=False, n=POIS_N, **params):
    """Oracle at POIS_P with the entries of `params` (Re, Ri, Prandtl, Lx) replaced."""
    from oracle.poiseuille import PoiseuilleCntsOracle, PoiseuilleOracle
    p = dict(POIS_P, **params)
    return (PoiseuilleCntsOracle if continuous else PoiseuilleOracle)(Nx, Nz, dt=POIS_DT, N_ITERS=n, s=s, delta=POIS_DELTA, **p)


def pois_input(Nx, Nz, continuous=False, seed=42):
    """synthetic_ic / 10 * synthetic_ic_cnts of the oracle at POIS_P (so the wavenumbers of its stream function are those of Lx = 7); made
    once per size and seed."""
    from oracle.poiseuille import synthetic_ic, synthetic_ic_cnts
    key = (Nx, Nz, continuous, seed)
    if key not in _POIS_X:
        o = pois_oracle(Nx, Nz, 0, continuous, n=1)
        _POIS_X[key] = 10. * synthetic_ic_cnts(o, seed) if continuous else synthetic_ic(o, seed)
        _POIS_X[key].setflags(write=False)
    return _POIS_X[key]


# ---- SH23 ------------------------------------------------------------------------------------------------------------------------------
SH23_CASES = [((0., 10.), 0.2), ((-3., 17.5), -1.7)]
SH23_DEFAULT = ((0., 12. * np.pi), -0.3)
SH23_DT, SH23_N = 0.1, 20
SH23_NPTS = [64, 54]                 # 64: the tuned kernels; 54: the any-length kernels


def sh23_input(Npts, seed=42):
    return 0.3 * np.random.RandomState(seed).standard_normal(2 * Npts)


def sh23_growth(L, a, m, dt):
    """Infinitesimal amplitude: factor per SBDF1 step of mode m of a box of length L."""
    km = 2. * np.pi * m / L
    return (1. / dt) / (1. / dt + (1. - km ** 2) ** 2 - a)


# ---- SHB23 -----------------------------------------------------------------------------------------------------------------------------
SHB23_CASES = [((-12., 15.), -0.4), ((0., 25.), 0.05)]
SHB23_DEFAULT = ((-20., 20.), -0.1)
SHB23_DT, SHB23_M0 = 1e-2, 0.0019
SHB23_DISCRETE_SIZES = [(64, 20), (50, 20), (512, 12)]      # (N, steps): tuned; the NH = 0 form; cluster mode
SHB23_CNTS_SIZES = [(32, 20), (256, 20)]                    # one workgroup; cluster mode
_SHB_X = {}


def shb23_oracle(N, n, interval, a, continuous=False):
    from oracle import shb23 as osh
    return (osh.SHB23CntsOracle if continuous else osh.SHB23Oracle)(N, interval=interval, dt=SHB23_DT, N_ITERS=n, a=a)


def shb23_input(N, interval, a, continuous=False, seed=42):
    """osh.synthetic_ic / synthetic_ic_cnts of the oracle built with that interval and a; made once per case."""
    from oracle import shb23 as osh
    key = (N, interval, a, continuous, seed)
    if key not in _SHB_X:
        o = shb23_oracle(N, 1, interval, a, continuous)
        _SHB_X[key] = (osh.synthetic_ic_cnts if continuous else osh.synthetic_ic)(o, seed, SHB23_M0)
        _SHB_X[key].setflags(write=False)
    return _SHB_X[key]


# ---- KDyn ------------------------------------------------------------------------------------------------------------------------------
KDYN_BAD_INTERVAL = (0., 4. * np.pi)
KDYN_GOOD_INTERVALS = [(0., 2. * np.pi), (1., 1. + 2. * np.pi)]
