"""Full-spectrum inputs and band-by-band comparison for SH23, SHB23 and Poiseuille (shared by test_bands_oracle_cpu.py, which shows on the
oracle alone that the cases are well posed and that the criterion sees what a whole-vector norm hides, and test_bands_gpu.py, which demands
the oracle's answer of the kernels in every band).

Every other oracle comparison of these three problems feeds a band-limited, pre-smoothed input (synthetic_ic / Generate_IC) and judges
one L2 norm over the whole vector, so the upper part of the spectrum carries 1e-3 .. 1e-25 of what is measured.  Here the input is white
noise on the grid of the flat vector (no filter, no preparatory steps), the step is small enough that every band survives the n steps,
and a vector is cut into K index bands of its spectral view (K x K rectangles for Poiseuille), each judged against its own norm:

    band_defects(got, ref, bands, floor)[b] = |got_b - ref_b| / max(|ref_b|, floor |ref|)

No band is left out: one that holds less than `floor` of the vector is still held `floor` times more sharply than a whole-vector norm would.
Tolerances are the suite's own (RTOL = 1e-6 for J, <X,g> and gradients, 1e-9 / 1e-8 for snapshots), FLOOR = 1e-3.

Spectral views.  SH23 and both Continuous formulations store coefficients; a gradient is a grid vector and goes, device's and oracle's
alike, through one host map per component: np.fft.rfft cut to the coefficient count (SH23), oracle.shb23.transform (SHB23 Discrete),
o.to_coeff (Continuous), o.transform (Poiseuille Discrete).  The SHB23 Discrete stack holds GRID states: they are judged in index bands
of the stored vector (space: the end bands are the rows next to the walls) and, through oracle.shb23.transform, in bands of the spectrum.

Imports numpy and the oracle only.
"""
import numpy as np

RTOL = 1e-6
FLOOR = 1e-3
SNAP_TOL = {"sh23": 1e-9, "shb23": 1e-8, "pois": 1e-8}
NORM2 = {"sh23": 0.0725, "shb23": 0.0019, "pois": 0.02}


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


# ---- bands -------------------------------------------------------------------------------------------------------------------------------
def bands_1d(n, K=4):
    """K equal index ranges over n coefficients."""
    e = np.linspace(0, n, K + 1).astype(int)
    return [(slice(e[i], e[i + 1]),) for i in range(K)]


def bands_2d(nx, nz, K=3):
    """K x K rectangles over an (nx, nz) coefficient array, x band slowest."""
    ex, ez = np.linspace(0, nx, K + 1).astype(int), np.linspace(0, nz, K + 1).astype(int)
    return [(slice(ex[i], ex[i + 1]), slice(ez[j], ez[j + 1])) for i in range(K) for j in range(K)]


def band_shares(ref, bands):
    """|ref_b| / |ref| per band."""
    ref = np.asarray(ref)
    tot = np.linalg.norm(ref)
    return [float(np.linalg.norm(ref[b]) / tot) for b in bands]


def band_defects(got, ref, bands, floor=FLOOR):
    """Per band |got_b - ref_b| / max(|ref_b|, floor |ref|): every band is judged, a small one against floor times the whole vector."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    tot = np.linalg.norm(ref)
    return [float(np.linalg.norm(got[b] - ref[b]) / max(np.linalg.norm(ref[b]), floor * tot)) for b in bands]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def white_input(kind, shape, seed, norm2=None, oracle=None):
    """Seeded standard_normal on the grid of the problem's flat vector, scaled with the oracle's own inner product to <X,X> = norm2 (the
    usual value of the problem when None).  No filter, no preparatory steps.
    kind: 'sh23' (shape = Npts; 2 Npts values), 'shb23' (N; N values), 'shb23c' (N modes; 2 N values), 'pois' ((Nx, Nz); 2 Nx Nz values),
    'poisc' ((Nx, Nz) modes; two fields on the 3/2 grid).  `oracle`: an oracle of that size whose inner product is used (else one is made)."""
    if oracle is None:
        oracle = make_oracle(kind, shape, 1)
    size = {"sh23": lambda: oracle.G, "shb23": lambda: oracle.N, "shb23c": lambda: oracle.G, "pois": lambda: 2 * oracle.Nx * oracle.Nz,
            "poisc": lambda: 2 * oracle.Gx * oracle.Gz}[kind]()
    x = np.random.RandomState(seed).standard_normal(size)
    x *= np.sqrt((NORM2[kind.rstrip("c")] if norm2 is None else norm2) / oracle.inner(x, x))
    x.setflags(write=False)
    return x


def make_oracle(kind, shape, n, dt=None, s=0):
    from oracle import poiseuille as opz, sh23 as osh23, shb23 as oshb
    if kind == "sh23":
        return osh23.SH23Oracle(shape, dt=sh23_dt(shape) if dt is None else dt, N_ITERS=n)
    if kind in ("shb23", "shb23c"):
        cont = kind == "shb23c"
        return (oshb.SHB23CntsOracle if cont else oshb.SHB23Oracle)(shape, dt=shb23_dt(shape, cont) if dt is None else dt, N_ITERS=n)
    cont = kind == "poisc"
    Nx, Nz = shape
    return (opz.PoiseuilleCntsOracle if cont else opz.PoiseuilleOracle)(Nx, Nz, Re=POIS_RE, Ri=POIS_RI, Prandtl=POIS_PR, delta=POIS_DELTA, s=s,
                                                                        dt=pois_dt(Nx, Nz, cont) if dt is None else dt, N_ITERS=n)


# ---- case tables ---------------------------------------------------------------------------------------------------------------------------
N_STEPS = 4
SEED, BATCH_SEEDS = 42, (42, 7, 3)

# SH23.  The step is the largest power of ten (at most 0.1) below 1 / (1 - k_max^2)^2: with 0.1 the top band of a white input is gone after
# two steps, with this rule the top mode loses at most a factor 2 per step.
SH23_L = 12. * np.pi
SH23_SIZES = [16, 21, 54, 96, 100, 112, 256, 1024, 1100]     # 21: odd; 21, 54: run-time length; radix 3, 5, 7; 1100: beyond 64 KB of LDS
SH23_ANY_SIZE = 64                                           # with SMO_SH_ANY=1
SH23_BATCH_SIZES = [64, 54]                                  # BATCH_SEEDS
SH23_HORIZONS = (64, (4, 2, 3))                              # member b: BATCH_SEEDS[b], its own number of steps
SH23_ADJOINTS = ("Discrete", "Continuous")


def sh23_dt(Npts):
    kmax = 2. * np.pi * (Npts // 2) / SH23_L
    return min(0.1, 10. ** np.floor(np.log10(1. / (1. - kmax ** 2) ** 2)))


# SHB23 Discrete: (N, steps) at dt = 1e-2
SHB23_SIZES = [20, 64, 96, 127, 256, 512, 1024, 1023]        # 127: prime; >= 256: the cluster; 1023: run-time length, remainder workgroup
SHB23_NO_CLUSTER = [256, 512, 1024, 1023]                    # also with SMO_SHB_CLUSTER=0
SHB23_ANY_SIZE = 512                                         # with SMO_SHB_ANY=1
SHB23_BATCH_SIZES = [64, 512]                                # 512: one workgroup per member at a size that alone takes the cluster
# SHB23 Continuous: the stack holds coefficients, and at dt = 1e-2 the top band of snapshot 4 is 3.5e-9 at 256 modes
SHB23C_SIZES = [32, 48, 64, 256, 333]
SHB23C_BATCH_SIZES = [256]


def shb23_dt(N, continuous=False):
    return 1e-5 if continuous and N >= 256 else 1e-2


# Poiseuille at the parameters of test_poiseuille_gpu.py.  (Nx, Nz, steps); the step is the largest of 5e-3, 1e-3, 1e-4 at which the oracle
# keeps FLOOR in every band of u and w (test_bands_oracle_cpu.py holds the oracle to that).
POIS_RE, POIS_RI, POIS_PR, POIS_DELTA = 500., 0.05, 1., 0.3
POIS_LADDER = (5e-3, 1e-3, 1e-4)
POIS_SIZES = [(24, 24, 3), (30, 66, 2), (48, 36, 4), (96, 48, 2),        # 30 x 66: ragged z tile, Nx with a factor 5
              (18, 15, 3), (42, 27, 3), (66, 33, 2), (54, 45, 2), (90, 21, 2)]       # odd Nz, and Nx without an x-FFT instantiation (dense x products)
POIS_VARIANT_SIZE = (30, 66, 2)
POIS_VARIANTS = [("SMO_POIS_APPLY", "dense"), ("SMO_POIS_XFFT", "0"), ("SMO_POIS_XPROD", "1")]     # and batch = 3, ckpt = 2
POISC_SIZES = [(16, 16, 3), (32, 24, 3)]
_POIS_DT = {(24, 24): 5e-3, (30, 66): 5e-3, (48, 36): 5e-3, (96, 48): 5e-3,       # the oracle keeps u and w above FLOOR at every value of the
            (18, 15): 5e-3, (42, 27): 5e-3, (66, 33): 5e-3, (54, 45): 5e-3, (90, 21): 5e-3}       # ladder (smallest share 1.8e-3, at 30 x 66), so: the
_POISC_DT = {(16, 16): 5e-3, (32, 24): 5e-3}                                      # largest


def pois_dt(Nx, Nz, continuous=False):
    return (_POISC_DT if continuous else _POIS_DT)[(Nx, Nz)]


# ---- spectral views ------------------------------------------------------------------------------------------------------------------------
def sh23_grad_view(o, g):
    return np.fft.rfft(np.asarray(g))[:o.Nc]


def shb23_grad_view(o, g, continuous):
    from oracle import shb23 as oshb
    return o.to_coeff(np.asarray(g)) if continuous else oshb.transform(np.asarray(g))


def pois_grad_views(o, g, continuous):
    """The two components, each as its own coefficient array: (ax, Nz) for the Discrete formulation (every carried wavenumber: the gradient
    is not de-aliased), (a, Nz) for the Continuous one."""
    if continuous:
        return [o.to_coeff(c) for c in o.split(g)]
    return [o.transform(c)[:o.ax] for c in o.split(g)]


# ---- the oracle's answers, once per case and process, read-only ------------------------------------------------------------------------------
_REF = {}


def _freeze(x):
    x = np.array(x)
    x.setflags(write=False)
    return x


def sh23_ref(Npts, n=N_STEPS, seed=SEED):
    """dict: X, dt, o (the oracle, its stack filled), J, snaps (Nc, n + 1), and per adjoint type g, ip = <X, g>, view."""
    key = ("sh23", Npts, n, seed)
    if key not in _REF:
        o = make_oracle("sh23", Npts, n)
        X = white_input("sh23", Npts, seed, oracle=o)
        r = dict(X=X, dt=o.dt, o=o, J=o.forward([X]), bands=bands_1d(o.Nc))
        r["snaps"] = _freeze(o.stack)
        for adj in SH23_ADJOINTS:
            g = _freeze(o.adjoint([X], adj)[0])
            r[adj] = dict(g=g, ip=o.inner(X, g), view=_freeze(sh23_grad_view(o, g)))
        _REF[key] = r
    return _REF[key]


def shb23_ref(N, continuous=False, n=N_STEPS, seed=SEED):
    """dict: X, dt, o, J, snaps (N, n + 1) as stored (Discrete: grid states), g, ip, view (the gradient's coefficients)."""
    key = ("shb23", N, continuous, n, seed)
    if key not in _REF:
        kind = "shb23c" if continuous else "shb23"
        base = _REF.get(("shb23", N, continuous, n, SEED))
        o = base["o"] if base else make_oracle(kind, N, n)                 # the tau operator is the cost of a case: one per size
        X = white_input(kind, N, seed, oracle=o)
        J = o.forward([X]); g = _freeze(o.adjoint([X])[0])
        _REF[key] = dict(X=X, dt=o.dt, o=o, J=J, snaps=_freeze(o.stack), g=g, ip=o.inner(X, g), view=_freeze(shb23_grad_view(o, g, continuous)),
                         bands=bands_1d(N))
    return _REF[key]


def shb23_snap_view(snap, continuous):
    """Coefficients of a stored snapshot."""
    from oracle import shb23 as oshb
    return np.asarray(snap) if continuous else oshb.transform(np.asarray(snap))


def pois_ref(Nx, Nz, n, s, continuous=False, seed=SEED, dt=None):
    """dict: X, dt, o, J, snaps {(field, i): (rows, Nz) coefficients for i in 0..n} (Discrete: every carried wavenumber, rows o.a.. exactly
    zero), g, ip, views (two coefficient arrays), bands_snap (over the retained rows), bands_grad, xkeep (rows the snapshot bands cover)."""
    key = ("pois", Nx, Nz, n, s, continuous, seed, dt)
    if key not in _REF:
        kind = "poisc" if continuous else "pois"
        o = make_oracle(kind, (Nx, Nz), n, dt=dt, s=s)
        X = white_input(kind, (Nx, Nz), seed, oracle=o)
        J = o.forward([X])
        rows = o.a if continuous else o.ax
        snaps = {(f, i): _freeze(o.stack[f, :rows, :, i]) for f in range(3) for i in range(n + 1)}
        g = _freeze(o.adjoint([X])[0])
        views = [_freeze(v) for v in pois_grad_views(o, g, continuous)]
        _REF[key] = dict(X=X, dt=o.dt, o=o, J=J, snaps=snaps, g=g, ip=o.inner(X, g), views=views, xkeep=o.a, bands_snap=bands_2d(o.a, Nz),
                         bands_grad=bands_2d(rows, Nz))
    return _REF[key]
