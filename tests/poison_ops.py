"""Results must not depend on what device memory held before: the case table and the runner of test_poison_gpu.py (test_poison_cpu.py holds
the table to the list of paths it has to name).

No allocation of the library is cleared: DevPool::alloc (every buffer of a context) and smo_vec_alloc (every device vector) hand out what
hipMalloc gives, and a solve may rely only on what it wrote itself.  In a test process nearly every block is a page the driver has just
cleared, so an unwritten element reads 0.0 — the one value for which a missing initialisation or an unmasked tail read gives the right
answer.  SMO_POISON=<byte> (csrc/common.cpp) fills every block with that byte before it is handed out; run(case, fill, monkeypatch) builds a
fresh domain and context under one fill, runs the case's sequence and returns every number it produced:

    1 forward   2 adjoint   3 <X, g>   4 every snapshot 0..n   5 forward and adjoint of a second input on the same context (buffers that are
    allocated at first use are reused here)   6 the first input again   7 (SH23 "hessvec" cases) two Hessian-vector products

FILLS: None (unset: what the suite sees elsewhere), 0x00, 0xFF (a NaN double, integer -1, unsigned 4294967295) and 0x3F (the finite double
0x3F3F3F3F3F3F3F3F ~ 4.8e-4, unsigned 1061109567: a read whose NaN a comparison, an fmax or a select would swallow still shifts the result).
The criterion is equality of bits with the unset run (the library promises fixed summation orders and no floating-point atomics), plus
equal path indicators (ctx.get), so that a fill cannot move a case onto another path unnoticed.

Inputs are the seeded ones of the neighbouring suites: kdyn.synthetic_field plus noise (symmetry_ops.kd_dirty_fields; above G = 96
symmetry_ops.kd_cheap_field, as in test_symmetry_gpu.py) and band_ops.white_input; time steps likewise (KDyn 1e-2, 1e-3 above G = 96;
band_ops.sh23_dt / shb23_dt; Poiseuille 5e-3).  Every case is the smallest shape at which its path still differs from its neighbours.

Imports numpy only; the library and the oracle (whose inner product scales the white inputs) are imported when a case runs.
"""
import numpy as np

FILLS = (None, 0x00, 0xFF, 0x3F)
FILL_IDS = ("unset", "0x00", "0xFF", "0x3F")

KD_RM, KD_N = 1.3, 3
KD_TWO = (("Integrated", "Continuous"), ("Final", "Discrete"))
KD_ALL4 = tuple((c, a) for c in ("Final", "Integrated") for a in ("Discrete", "Continuous"))
KD_TUNED = (8, 16, 20, 28, 36)                 # G = 12, 24, 30, 42, 54: radix 2 / 3 / 5 / 7 and a repeated 3
KD_ANY = (6, 10, 22)                           # G = 9, 15, 33: run-time length; odd G with the unpaired last line
KD_LARGE = (128, 256)                          # G = 192, 384: half tiles, half twiddle table, narrower adjoint x tiles
KD_BATCH_RM, KD_BATCH_HZ = (0.7, 1.3, 2.9), (3, 1, 2)
# Ty at N = 16: another padding of its planes, the plane layout (G = 24 takes the z-block layout by default: KDynEnv, pick_ty_layout), and the
# adjoint x pass with both field groups in the tile at once
KD_TY_KNOBS = (("SMO_KD_TYPAD", "24"), ("SMO_KD_TYL", "0"), ("SMO_KD_ADJ_SEQ", "0"))
SH_HESS_SIZES = (64, 54, 1024)                 # Hessian-vector products: tuned, run-time length, above 768 (two rounds of two transforms)
SH_N, SHB_N, PZ_N = 4, 4, 3
SH_SIZES = (16, 21, 54, 64, 1100)              # 21, 54: run-time length; 1100: above 64 KB of LDS
SH_ADJ = ("Discrete", "Continuous")
SH_HZ = (4, 2, 3)
SH_A = (0.2, -1.7, -0.3)
SHB_SIZES = (20, 64, 127, 256, 1023)           # 256: the cluster; 1023: run-time length with the remainder workgroup
SHBC_SIZES = (32, 256)
PZ_SIZES = ((12, 12), (24, 24), (18, 15), (30, 66), (42, 27))      # below one tile, odd Nz, a ragged z tile, an Nx without an x FFT
PZC_SIZES = ((16, 16), (32, 24))
PZ_VARIANT = (30, 66)
PZ_RE, PZ_RI, PZ_PR, PZ_DELTA, PZ_DT = 500., 0.05, 1., 0.3, 5e-3
SEEDS = ((42, 7, 3), (5, 11, 13))              # first and second input of member b
VEC_SIZES = (1, 7, 1001)


def _case(family, size, variant="plain", **kw):
    c = dict(family=family, size=size, variant=variant, env={}, n=None)
    c.update(kw)
    return c


def _kd(N, combos, variant="plain", n=KD_N, **kw):
    return [_case("kdyn", N, variant, n=n, cost=c, adj=a, **kw) for c, a in combos]


def _cases():
    out = []
    # ---- KDyn ------------------------------------------------------------------------------------------------------------------------
    for N in KD_TUNED + KD_ANY:
        out += _kd(N, KD_ALL4 if N in (8, 10) else KD_TWO)
    out += _kd(16, KD_TWO, "SMO_KD_ANY=1", env={"SMO_KD_ANY": "1"})
    out += _kd(16, KD_TWO, "ckpt=3", n=7, ckpt=3)
    out += _kd(16, KD_TWO, "SMO_KD_DENSE_FROM=4", n=9, ckpt=2, env={"SMO_KD_DENSE_FROM": "4"})
    for name in ("SMO_KD_TYSTACK", "SMO_KD_FUSE_NEXT", "SMO_KD_GRAPH"):
        out += _kd(16, KD_TWO, name + "=0", env={name: "0"})
    for name, value in KD_TY_KNOBS:
        out += _kd(16, KD_TWO, "%s=%s" % (name, value), env={name: value})
    out += _kd(16, KD_TWO, "ckpt=3,SMO_KD_TYCACHE=0", n=7, ckpt=3, env={"SMO_KD_TYCACHE": "0"})
    out += _kd(24, KD_TWO, "graph", n=8, replays=True)
    out += _kd(16, KD_TWO, "batch=3", batch=3, rm=KD_BATCH_RM, hz=KD_BATCH_HZ)
    out += _kd(16, KD_TWO, "frozen_U", frozen=True, keep=True)
    out += _kd(16, (("Final", "Discrete"),), "frozen_U,keep_states=False", frozen=True, keep=False)
    out += [_case("kdyn", 16, "gram", op="gram", batch=3, rm=KD_BATCH_RM, hz=KD_BATCH_HZ, n=KD_N, cost="Final")]
    out += [_case("kdyn", N, "transform", op="transform", n=1, cost="Final") for N in (16, 10)]
    out += _kd(16, KD_TWO, "devices=[0,0]", devices=(0, 0))
    for N in KD_LARGE:
        out += _kd(N, (("Final", "Discrete"),), n=2)
    # ---- SH23 ------------------------------------------------------------------------------------------------------------------------
    for N in SH_SIZES:
        out += [_case("sh23", N, n=SH_N, adj=a) for a in SH_ADJ]
    out += [_case("sh23", 64, "SMO_SH_ANY=1", n=SH_N, adj=a, env={"SMO_SH_ANY": "1"}) for a in SH_ADJ]
    out += [_case("sh23", 54, "batch=3", n=SH_N, adj=a, batch=3) for a in SH_ADJ]
    out += [_case("sh23", 64, "horizons", n=SH_N, adj=a, batch=3, hz=SH_HZ) for a in SH_ADJ]
    out += [_case("sh23", 64, "a per member", n=SH_N, adj=a, batch=3, a=SH_A) for a in SH_ADJ]
    out += [_case("sh23", 54, "gram", op="gram", n=SH_N, batch=3)]
    out += [_case("sh23", N, "hessvec", n=SH_N, adj="Discrete", hessvec=True) for N in SH_HESS_SIZES]
    out += [_case("sh23", 64, "hessvec,horizons", n=SH_N, adj="Discrete", batch=3, hz=SH_HZ, hessvec=True)]
    # ---- SHB23 -----------------------------------------------------------------------------------------------------------------------
    out += [_case("shb23", N, n=SHB_N) for N in SHB_SIZES]
    out += [_case("shb23", 256, "SMO_SHB_CLUSTER=0", n=SHB_N, env={"SMO_SHB_CLUSTER": "0"})]
    out += [_case("shb23", 64, "SMO_SHB_ANY=1", n=SHB_N, env={"SMO_SHB_ANY": "1"})]
    out += [_case("shb23", N, "continuous", n=SHB_N, continuous=True) for N in SHBC_SIZES]
    out += [_case("shb23", N, "batch=3", n=SHB_N, batch=3) for N in (64, 512)]
    out += [_case("shb23", N, "transform", op="transform", n=1) for N in (20, 127)]
    # ---- Poiseuille --------------------------------------------------------------------------------------------------------------------
    for s in (0, 1):
        out += [_case("pois", sz, n=PZ_N, s=s) for sz in PZ_SIZES]
        out += [_case("pois", sz, "continuous", n=PZ_N, s=s, continuous=True) for sz in PZC_SIZES]
        for name, value in (("SMO_POIS_APPLY", "dense"), ("SMO_POIS_XFFT", "0"), ("SMO_POIS_XPROD", "1"), ("SMO_POIS_HODLR_SPLIT", "3")):
            out += [_case("pois", PZ_VARIANT, "%s=%s" % (name, value), n=PZ_N, s=s, env={name: value})]
        out += [_case("pois", PZ_VARIANT, "ckpt=2", n=PZ_N, s=s, ckpt=2)]
        out += [_case("pois", PZ_VARIANT, "batch=3,SMO_POIS_APPLY_MB=%d" % mb, n=PZ_N, s=s, batch=3, env={"SMO_POIS_APPLY_MB": str(mb)}) for mb in (1, 2, 4)]
    out += [_case("pois", (18, 15), "transform", op="transform", n=1, s=0)]
    for c in out:
        c["id"] = case_id(c)
    return out


def case_id(c):
    size = "%dx%d" % c["size"] if isinstance(c["size"], tuple) else str(c["size"])
    parts = [c["family"], size]
    if c["variant"] != "plain":
        parts.append(c["variant"].replace(" ", "_"))
    for key in ("cost", "adj"):
        if c.get(key) and c.get("op") is None:
            parts.append(c[key])
    if "s" in c and c.get("op") is None:
        parts.append("s%d" % c["s"])
    return "-".join(parts)


CASES = _cases()


def coverage(cases=None):
    """{(family, size, variant): sorted list of the (cost, adjoint type) / adjoint type / s values the table runs it with}."""
    cov = {}
    for c in (CASES if cases is None else cases):
        if c["family"] == "kdyn":
            what = (c.get("cost"), c.get("adj"))
        elif c["family"] == "sh23":
            what = c.get("adj")
        elif c["family"] == "pois":
            what = c["s"]
        else:
            what = None
        cov.setdefault((c["family"], c["size"], c["variant"]), []).append(what)
    return {k: sorted(v, key=repr) for k, v in cov.items()}


# ---- inputs: made once per shape, shared by the four fills, read-only -------------------------------------------------------------------------
_INPUTS = {}


def _frozen(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    x.setflags(write=False)
    return x


def _cached(key, make):
    if key not in _INPUTS:
        _INPUTS[key] = make()
    return _INPUTS[key]


def kd_dt(G):
    return 1e-2 if G <= 96 else 1e-3


def kd_inputs(G, member=0):
    """[(B, U) first, (B, U) second]: test_kdyn_gpu._fields(dirty=True) with the seeds moved on by the member and the input; above G = 96 the
    inputs of test_symmetry_gpu.py, which need no host FFT (the second one changes B only)."""
    def make():
        import symmetry_ops as so
        if G > 96:
            B, U = so.kd_cheap_field(G, 9), so.kd_cheap_field(G, 10, mean=0.)
            return [(_frozen(B), _frozen(U)), (_frozen(so.kd_cheap_field(G, 11, mean=0.02)), _frozen(U))]
        from spheremanopt_amd import kdyn
        out = []
        for k in range(2):
            sd = 4 * member + 2 * k
            if sd == 0:
                B, U = so.kd_dirty_fields(G, kdyn.synthetic_field)
            else:
                B = kdyn.synthetic_field(G, 1 + sd) + 0.2 * np.random.RandomState(9 + sd).standard_normal(3 * G ** 3) + 0.05
                U = kdyn.synthetic_field(G, 2 + sd) + 0.2 * np.random.RandomState(10 + sd).standard_normal(3 * G ** 3)
            out.append((_frozen(B), _frozen(U)))
        return out
    return _cached(("kdyn", G, member), make)


def white_inputs(kind, shape, members=1):
    """[first, second] input, each the members' band_ops.white_input concatenated."""
    def make():
        import band_ops as bo
        o = bo.make_oracle(kind, shape, 1, dt=PZ_DT if kind.startswith("pois") else None)
        return [_frozen(np.concatenate([bo.white_input(kind, shape, SEEDS[k][b], oracle=o) for b in range(members)])) for k in range(2)]
    return _cached((kind, shape, members), make)


# ---- the runner ----------------------------------------------------------------------------------------------------------------------------------
def set_fill(monkeypatch, fill):
    if fill is None:
        monkeypatch.delenv("SMO_POISON", raising=False)
    else:
        monkeypatch.setenv("SMO_POISON", str(int(fill)))


def run(case, fill, monkeypatch):
    """One case under one fill on a fresh domain and context -> (values, paths): every number the sequence produced as a flat list of arrays,
    and the path indicators of the context.  The contexts are dropped and the vector pool is released before it returns."""
    from spheremanopt_amd import devvec
    for name, value in case["env"].items():
        monkeypatch.setenv(name, value)
    set_fill(monkeypatch, fill)
    try:
        return _RUNNERS[case["family"]](case)
    finally:
        devvec.release_pool()
        for name in case["env"]:
            monkeypatch.delenv(name, raising=False)
        monkeypatch.delenv("SMO_POISON", raising=False)


def _arr(x):
    return np.atleast_1d(np.asarray(x))


def _sequence(ctx, inputs, adj, snapshots, inner_with=lambda X, g: [(X[c], g[c]) for c in range(len(g))]):
    """Steps 1 - 6 on one context.  inputs: [first, second], each the list of the context's vectors; snapshots() -> the (index, member)
    pairs the stack holds after a forward solve."""
    out = []
    for k, X in enumerate((inputs[0], inputs[1], inputs[0])):
        out.append(_arr(ctx.forward(list(X))))
        g = ctx.adjoint(None, adj)
        out += list(g)
        if k == 0:
            out += [_arr(ctx.inner(x, y)) for x, y in inner_with(X, g)]
            out += [ctx.snapshot(i, b) for i, b in snapshots()]
    return out


def _gram_ops(ctx, x, y):
    """gram / combine on host vectors and on device vectors: [B][vec_len] inputs x, y."""
    from spheremanopt_amd.devvec import DeviceVector
    B = ctx.batch
    Cm = np.random.RandomState(17).standard_normal((B, B))
    xd, yd = DeviceVector.from_numpy(x, ctx.cfg.device), DeviceVector.from_numpy(y, ctx.cfg.device)
    out = [ctx.gram(x), ctx.gram(x, y), ctx.combine(Cm, x), ctx.gram_dev(xd), ctx.gram_dev(xd, yd), ctx.combine_dev(Cm, xd).numpy()]
    del xd, yd
    return out


def _run_kdyn(c):
    from spheremanopt_amd import kdyn
    N, n, B = c["size"], c["n"], c.get("batch", 1)
    G = 3 * N // 2
    dom = kdyn.KDynDomain(N, ckpt=c.get("ckpt", 1), devices=list(c["devices"]) if c.get("devices") else None)
    try:
        members = [kd_inputs(G, b) for b in range(B)]
        inputs = [[_frozen(np.concatenate([m[k][comp] for m in members])) if B > 1 else members[0][k][comp] for comp in range(2)] for k in range(2)]
        hz = c.get("hz")
        kw = dict(frozen_U=True, keep_states=c["keep"]) if c.get("frozen") else {}
        ctx = dom.context(c.get("rm", KD_RM), kd_dt(G), hz if hz else n, c["cost"], batch=B, **kw)
        if c.get("op") == "transform":
            out = []
            for k in (0, 1, 0):
                coeff = ctx.transform(0, inputs[k][0], out_len=ctx.snapshot_len)
                out += [coeff, ctx.transform(1, coeff, out_len=ctx.vec_len)]
        elif c.get("op") == "gram":
            out = []
            for k in (0, 1, 0):
                out += _gram_ops(ctx, inputs[k][0], inputs[k][1])
        else:
            def snapshots():
                if ctx.snapshot_len == 0:                               # a multi-device context keeps its snapshots distributed
                    return []
                if c.get("keep") is False:                              # no stack: the last state only
                    return [((hz[b] if hz else n), b) for b in range(B)]
                return [(i, b) for b in range(B) for i in range((hz[b] if hz else n) + 1)]
            out = _sequence(ctx, inputs, c["adj"], snapshots)
        paths = tuple(ctx.get(k) for k in (0, 1, 2, 5))
        if c.get("replays"):
            assert paths[2] > 0, "the solves were not replayed from captured graphs"
        return out, paths
    finally:
        dom.drop_contexts()


def _run_sh23(c):
    from spheremanopt_amd import _capi, sh23
    import band_ops as bo
    Npts, n, B = c["size"], c["n"], c.get("batch", 1)
    inputs = white_inputs("sh23", Npts, B)
    dom = sh23.SH23Domain(Npts)
    ctx = None
    try:
        if c.get("a"):
            ctx = _capi.Context(_capi.SMO_SH23, Npts, dom.interval, bo.sh23_dt(Npts), n, c["a"])
        else:
            ctx = dom.context(bo.sh23_dt(Npts), c["hz"] if c.get("hz") else n, batch=B)
        if c.get("op") == "gram":
            out = []
            for k in (0, 1, 0):
                out += _gram_ops(ctx, inputs[k], inputs[1 - k])
        else:
            hz = c.get("hz")
            out = _sequence(ctx, [[inputs[0]], [inputs[1]]], c["adj"], lambda: [(i, b) for b in range(B) for i in range((hz[b] if hz else n) + 1)])
            if c.get("hessvec"):                                        # 7 two directions at the point of the last forward solve (the tangent stack
                for V in (inputs[1], inputs[0]):                        #   is allocated by the first product)
                    (HV,), dJ = ctx.hessvec([V])
                    out += [HV, _arr(dJ)]
        return out, (ctx.get(0),)
    finally:
        if c.get("a") and ctx is not None:
            ctx.close()
        dom.drop_contexts()


def _run_shb23(c):
    from spheremanopt_amd import shb23
    import band_ops as bo
    N, n, B, cont = c["size"], c["n"], c.get("batch", 1), bool(c.get("continuous"))
    dom = shb23.SHBDomain(N, dealias=2 if cont else 1)
    try:
        ctx = dom.context(bo.shb23_dt(N, cont), n, batch=B)
        if c.get("op") == "transform":
            xs = [_frozen(np.random.RandomState(sd).standard_normal(N)) for sd in SEEDS[0][:2]]
            out = [ctx.transform(which, xs[k]) for k in (0, 1, 0) for which in range(4)]
        else:
            inputs = white_inputs("shb23c" if cont else "shb23", N, B)
            out = _sequence(ctx, [[inputs[0]], [inputs[1]]], "Continuous" if cont else "Discrete", lambda: [(i, b) for b in range(B) for i in range(n + 1)])
        return out, (ctx.get(1), ctx.get(2))
    finally:
        dom.drop_contexts()


def _run_pois(c):
    from spheremanopt_amd import poiseuille as pz
    (Nx, Nz), n, B, cont = c["size"], c["n"], c.get("batch", 1), bool(c.get("continuous"))
    dom = pz.PoiseuilleDomain(Nx, Nz, continuous=cont, ckpt=c.get("ckpt", 1))
    try:
        ctx = dom.context(PZ_RE, PZ_RI, n, PZ_DT, c["s"], PZ_PR, PZ_DELTA, batch=B)
        if c.get("op") == "transform":
            rs = np.random.RandomState(SEEDS[0][0])
            grids = [rs.standard_normal((Nx, Nz)) for _ in range(2)]
            coeffs = [rs.standard_normal((dom.a, Nz)) + 1j * rs.standard_normal((dom.a, Nz)) for _ in range(2)]
            for z in coeffs:
                z[0] = z[0].real                                        # the mean mode of a real field
            fns = (pz.transform, pz.transformInverse, pz.transformAdjoint, pz.transformInverseAdjoint)
            out = [np.ascontiguousarray(fns[which]((coeffs if which in (1, 2) else grids)[k], dom)).view(np.float64) for k in (0, 1, 0) for which in range(4)]
            return out, (dom.any_context().get(0),)
        inputs = white_inputs("poisc" if cont else "pois", (Nx, Nz), B)
        out = _sequence(ctx, [[inputs[0]], [inputs[1]]], "Continuous" if cont else "Discrete", lambda: [(i, b) for b in range(B) for i in range(n + 1)])
        return out, (ctx.get(0),)
    finally:
        dom.drop_contexts()


_RUNNERS = {"kdyn": _run_kdyn, "sh23": _run_sh23, "shb23": _run_shb23, "pois": _run_pois}


# ---- device vectors --------------------------------------------------------------------------------------------------------------------------------
def vector_algebra(n):
    """[(device result, NumPy's)] of a*X + b*Y, -X, deepcopy and smo_vec_axpby on a view at an odd element offset."""
    import copy
    import ctypes as C
    from spheremanopt_amd import _capi
    from spheremanopt_amd.devvec import DeviceVector
    rs = np.random.RandomState(n)
    x, y = rs.standard_normal(n + 1), rs.standard_normal(n + 1)
    a, b = 1.25, -0.3333333333333333
    X, Y = DeviceVector.from_numpy(x), DeviceVector.from_numpy(y)
    pairs = [((a * X + b * Y).numpy(), a * x + b * y), ((-X).numpy(), -x), (copy.deepcopy(X).numpy(), x)]
    O = DeviceVector(n + 1)
    _capi._check(_capi.lib().smo_vec_axpby(0, n, a, C.c_void_p(X.ptr + 8), b, C.c_void_p(Y.ptr + 8), C.c_void_p(O.ptr + 8)))
    pairs.append((O.numpy()[1:], a * x[1:] + b * y[1:]))
    return pairs


def fill_pattern(fill, n):
    """n doubles whose every byte is `fill`."""
    return np.full(8 * n, fill, dtype=np.uint8).view(np.float64)


def same_bits(a, b):
    """Bit-for-bit equality (NaN payloads included: np.array_equal does not hold NaN == NaN)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
