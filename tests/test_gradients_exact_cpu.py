"""The premises of tests/test_gradients_exact_gpu.py, pinned on the CPU oracles (tests/exact_grad_ops.py states them), and the three places
where the reference's Discrete adjoints are NOT exact gradients, characterised so that nobody "fixes" them.  No GPU.

Exact (asserted with the bound of exact_ops.needle_defect, JTOL = 1e-12 on every J of the stencil plus GTOL = 1e-11 on |g| |d|, which must
stay below SHARE = 1e-8 of |g| |d|); figures are shares of |g| |d| on the oracle, white inputs, |d| = 0.1 |X|:
    SH23, every horizon and size       defect <= 1.5e-15 (n = 1 and 2, Npts 16 .. 1100), bound 1.6e-11 .. 2.1e-11; out of the band
                                       |<g, d>| is within the bound and J(X + t d) within JTOL |J| of J(X)
    Poiseuille s = 0, ONE step         Ri = 0, u and w needles, and Ri = 0.05, u needles: defect <= 1.1e-15, bound 1.5e-11
                                       (Ri = 0.05, w needles: up to 2.0e-10 at 18 x 15 — step 0 reads the analytic derivative of the base profile, the
                                       adjoint Dz rho_0; not asserted, not used on the device)
    SH23 Hessian identity              <W, HV> = stencil of <g(X + j V), W> on hessvec_ops: defect <= 1e-15 of |HV| |W|, bound 1.8e-10 ..
                                       3.2e-10 at |V| = 0.1 |X|, so SH23_HESSIAN_H = 0.1
A 1e-8 relative error planted in one coefficient fails the needle at that coefficient and passes every other needle.

Not exact, by the reference's design (the subclasses that repair two of them live in this file; oracle/ keeps the reference's behaviour):
    Poiseuille, N_ITERS >= 2           worst needle 1.5e-5 .. 3.3e-4 of |g| |d| (24 x 24, 18 x 15; n = 2, 3): the adjoint re-derives uz, wz, rz
                                       as Dz of the stored u, w, rho (oracle/poiseuille.py adjoint, FWD_Solve_Poiseuille.py:1620-1626) where
                                       the forward products read the tau solve's own.  Handing the solved derivatives to the adjoint:
                                       <= 9.7e-16 at N_ITERS = 2, 3, and not a bit of difference at N_ITERS = 1.
    SHB23                              1.2e-6 .. 6.3e-4 at N_ITERS = 1, 2 (N = 20, 64): the adjoint has no transpose of the de-aliasing mask
                                       (oracle/shb23.py adjoint, FWD_Solve_SHB23.py:842-845).  With the mask applied to r: <= 2.5e-15.
    Poiseuille, out of the band        J is blind to the direction (|J(X + t d) - J(X)| <= JTOL |J|), the gradient is not (|<g, d>| is
                                       1.2e-6 .. 1.5e-2 of |g| |d|).
    Poiseuille s = 1, ONE step         J does not depend on u, and depends on w through the base profile's derivative alone (analytic in the
                                       forward solve, Dz rho_0 in the adjoint): the w needles miss by 3e-4 (24 x 24), 2e-12 (30 x 66), 1e-2
                                       (18 x 15), 8e-5 (42 x 27) at every step of the ladder, and the bound is 1.6e-8 (h = 0.1), 5.4e-9 (0.3),
                                       1.6e-9 (1.0).  No step qualifies: POIS_MIXNORM_H = None, no s = 1 case on the device.
The oracle of the largest device case, 384 x 192, is left out here: its 128 tau systems of 1345 unknowns alone take longer than this file may.
"""
import numpy as np
import pytest

import band_ops as bo
import exact_grad_ops as eg
import hessvec_ops as ho
from exact_ops import GTOL, JTOL, RTOL, SHARE
from oracle import shb23 as oshb
from oracle.poiseuille import PoiseuilleOracle
from oracle.sh23 import SH23Oracle

SEED = 42
SH23_CASES = [(N, 1) for N in bo.SH23_SIZES + [bo.SH23_ANY_SIZE]] + [(N, 2) for N in (16, 54, 256, 1100)]
POIS_SIZES = [(24, 24), (30, 66), (18, 15), (42, 27), (96, 48), (90, 21)]
POIS_CASES = [(s, Ri, "u") for s in POIS_SIZES for Ri in (bo.POIS_RI,)] + [(s, 0., "uw") for s in POIS_SIZES]
_PRINT = "%-34s defect %.1e  bound %.1e  of |g||d|"


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


def _lines(o, X, dirs, m, h, ip):
    """{name: (in_band, d, [J at line_points])}"""
    out = {}
    for name, inside, du in dirs:
        d = eg.scaled(du, X, h, ip)
        out[name] = (inside, d, [o.forward([Y]) for Y in eg.line_points(X, d, m)])
    return out


def _assert_exact(tag, g, lines, m, ip):
    worst = (0., 0.)
    for name, (inside, d, Js) in lines.items():
        if inside:
            defect, bound, gd = eg.line_defect(g, d, m, Js, ip)
            worst = max(worst[0], defect / gd), max(worst[1], bound / gd)
            assert defect <= bound, (tag, name, defect / gd, bound / gd)
            assert bound < SHARE * gd, (tag, name, bound / gd)
    print(_PRINT % ((tag,) + worst))


# ---- the helpers themselves ------------------------------------------------------------------------------------------------------------
def test_degree_half_width():
    assert [eg.degree_half_width("sh23", n) for n in (1, 2, 3)] == [3, 9, 27]
    assert [eg.degree_half_width("pois", n) for n in (1, 2, 3)] == [2, 4, 8]


@pytest.mark.parametrize("Nx,Nz", POIS_SIZES + [(384, 192)])
def test_host_inner_product_is_the_oracles(Nx, Nz):
    o = PoiseuilleOracle(Nx, Nz, N_ITERS=1)
    ip = eg.pois_inner_product(Nx, Nz)
    rs = np.random.RandomState(1)
    x, y = rs.standard_normal(2 * Nx * Nz), rs.standard_normal(2 * Nx * Nz)
    for a, b in ((x, y), (x, x)):
        size = o.inner(np.abs(a), np.abs(b))
        assert abs(ip(a, b) - o.inner(a, b)) <= 1e-15 * size
    assert eg.sh23_inner(x, y) == SH23Oracle(Nx * Nz, N_ITERS=1).inner(x, y)
    X = eg.white(2 * Nx * Nz, SEED, eg.POIS_NORM2, ip)
    assert _rel(X, bo.white_input("pois", (Nx, Nz), SEED, oracle=o)) < 1e-15 and (eg.POIS_NORM2, eg.SH23_NORM2) == (bo.NORM2["pois"], bo.NORM2["sh23"])


@pytest.mark.parametrize("Npts", [16, 21, 54])
def test_an_sh23_needle_is_one_fourier_coefficient(Npts):
    o = SH23Oracle(Npts, N_ITERS=1)
    inside, outside = eg.sh23_wavenumbers(Npts)
    assert len(set(inside)) == 6 and {0, 1, o.Nc // 2, o.Nc - 1} <= set(inside) and max(inside) == o.Nc - 1 and min(outside) >= o.Nc
    dirs = eg.sh23_directions(Npts)
    assert [n for n, _, _ in dirs] == ["k=%d" % k for k in inside + outside] + ["white"]
    for (name, inb, d), k in zip(dirs, inside + outside):
        assert abs(eg.sh23_inner(d, d) - 1.) < 1e-14 and inb == (k in inside)
        c = np.fft.rfft(d) / o.G
        assert abs(c[k]) > 0.3
        c[k] = 0.
        assert np.abs(c).max() < 1e-14, name
        assert (np.abs(o.to_coeff(d)).max() > 0.3) == inb               # the forward solve sees the in-band ones only


@pytest.mark.parametrize("Nx,Nz", [(24, 24), (18, 15), (30, 66)])
def test_a_poiseuille_needle_is_one_coefficient(Nx, Nz):
    o = PoiseuilleOracle(Nx, Nz, N_ITERS=1)
    assert eg.pois_band(Nx, Nz) == (o.a, o.Nz0)
    inside, outside = eg.pois_wavenumbers(Nx, Nz)
    assert len(set(inside)) == 10 and all(kx < o.a and kz < o.Nz0 for kx, kz in inside)
    assert set(eg.pois_wavenumbers(Nx, Nz, "corners")[0]) == {(0, 0), (o.a - 1, 0), (0, o.Nz0 - 1), (o.a - 1, o.Nz0 - 1)} < set(inside)
    assert any(0 < kx < o.a - 1 and 0 < kz < o.Nz0 - 1 for kx, kz in inside[8:])
    ip = eg.pois_inner_product(Nx, Nz)
    dirs = eg.pois_directions(Nx, Nz)
    assert len(dirs) == 24
    for (name, inb, d), (c, (kx, kz)) in zip(dirs, [(c, k) for c in (0, 1) for k in inside + outside]):
        assert abs(ip(d, d) - 1.) < 1e-14
        fields = [o.transform(f) for f in o.split(d)]
        assert not np.any(fields[1 - c])
        C = fields[c]
        assert abs(C[kx, kz]) > 0.05, name
        assert np.abs(o.DA * C).max() > 0.05 if inb else np.abs(o.DA * C).max() < 1e-14
        C[kx, kz] = 0.
        C[-kx, kz] = 0.
        assert np.abs(C).max() < 1e-13, name
    v = np.random.RandomState(2).standard_normal(2 * Nx * Nz)
    ref = np.concatenate([np.real(o.transformInverse(o.DA * o.transform(f))).ravel() for f in o.split(v)])
    assert _rel(eg.pois_band_project(v, Nx, Nz), ref) < 1e-13
    assert not np.any(eg.pois_band_project(v, Nx, Nz, "u").reshape(2, -1)[1])


# ---- SH23: exact at every horizon and size -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=SH23_CASES, ids=lambda p: "Npts%d-n%d" % p)
def sh(request):
    Npts, n = request.param
    o = SH23Oracle(Npts, dt=bo.sh23_dt(Npts), N_ITERS=n)
    X = eg.white(o.G, SEED, eg.SH23_NORM2, eg.sh23_inner)
    o.forward([X])
    g = o.adjoint([X], "Discrete")[0]
    m = eg.degree_half_width("sh23", n)
    dirs = eg.sh23_directions(Npts) + [("aligned", True, eg.unit(g, eg.sh23_inner))]
    return "SH23 %d n=%d" % (Npts, n), o, X, g, m, _lines(o, X, dirs, m, eg.H, eg.sh23_inner)


def test_sh23_discrete_adjoint_is_the_exact_gradient(sh):
    tag, o, X, g, m, lines = sh
    _assert_exact(tag, g, lines, m, eg.sh23_inner)


def test_sh23_gradient_has_no_content_out_of_the_band(sh):
    tag, o, X, g, m, lines = sh
    J0 = o.forward([X])
    for name, (inside, d, Js) in lines.items():
        if not inside:
            gd_, st, bound, jscale = eg.blind_defect(g, d, m, Js, eg.sh23_inner)
            assert gd_ <= bound and st <= jscale, (name, gd_, st, bound, jscale)
            assert max(abs(J - J0) for J in Js) <= JTOL * abs(J0)


def test_sh23_a_planted_error_of_1e_8_in_one_coefficient(sh):
    """g + 1e-8 |g| d_k fails needle k and passes every other needle; the norm comparison at RTOL accepts it."""
    tag, o, X, g, m, lines = sh
    names = [n for n, (inside, _, _) in lines.items() if inside and n.startswith("k=")]
    for bad_name in names:
        du = eg.unit(lines[bad_name][1], eg.sh23_inner)
        bad = g + 1e-8 * np.sqrt(eg.sh23_inner(g, g)) * du
        assert _rel(bad, g) < RTOL
        for name in names:
            defect, bound, gd = eg.line_defect(bad, lines[name][1], m, lines[name][2], eg.sh23_inner)
            assert (defect > bound) == (name == bad_name), (bad_name, name, defect / gd, bound / gd)


def test_sh23_a_narrower_stencil_is_not_exact():
    """Why the half-width matters: with m = 3 where the degree asks for 9 the needle misses by far more than its bound."""
    o = SH23Oracle(16, dt=0.1, N_ITERS=2)
    X = eg.white(o.G, SEED, eg.SH23_NORM2, eg.sh23_inner)
    o.forward([X])
    g = o.adjoint([X], "Discrete")[0]
    lines = _lines(o, X, eg.sh23_directions(16)[:2], 3, eg.H, eg.sh23_inner)
    for name, (_, d, Js) in lines.items():
        defect, bound, gd = eg.line_defect(g, d, 3, Js, eg.sh23_inner)
        assert defect > bound, (name, defect / gd, bound / gd)


# ---- Poiseuille, one step ------------------------------------------------------------------------------------------------------------------
def _pois_oracle(Nx, Nz, n, Ri, s=0, cls=PoiseuilleOracle, Re=bo.POIS_RE):
    return cls(Nx, Nz, Re=Re, Ri=Ri, Prandtl=bo.POIS_PR, delta=bo.POIS_DELTA, s=s, dt=5e-3, N_ITERS=n)


def _pois_base(o, comps, which="all", h=eg.H, out_of_band=True):
    Nx, Nz = o.Nx, o.Nz
    ip = eg.pois_inner_product(Nx, Nz)
    X = eg.white(2 * Nx * Nz, SEED, eg.POIS_NORM2, ip)
    J0 = o.forward([X])
    g = o.adjoint([X])[0]
    m = eg.degree_half_width("pois", o.N_ITERS)
    dirs = [d for d in eg.pois_directions(Nx, Nz, comps, which) if out_of_band or d[1]]
    dirs.append(("aligned", True, eg.unit(eg.pois_band_project(g, Nx, Nz, comps), ip)))
    return X, J0, g, m, ip, _lines(o, X, dirs, m, h, ip)


@pytest.fixture(scope="module", params=POIS_CASES, ids=lambda p: "%dx%d-Ri%g-%s" % (p[0] + p[1:]))
def pz(request):
    (Nx, Nz), Ri, comps = request.param
    o = _pois_oracle(Nx, Nz, 1, Ri)
    return ("Poiseuille %dx%d Ri=%g %s" % (Nx, Nz, Ri, comps), o) + _pois_base(o, comps)


def test_poiseuille_one_step_adjoint_is_the_exact_gradient(pz):
    tag, o, X, J0, g, m, ip, lines = pz
    _assert_exact(tag, g, lines, m, ip)


def test_poiseuille_cost_is_blind_out_of_the_band_and_the_gradient_is_not(pz):
    """Quirk 3: |J(X + t d) - J(X)| <= JTOL |J| for a needle out of the de-aliased band, while <g, d> != 0."""
    tag, o, X, J0, g, m, ip, lines = pz
    seen = 0
    for name, (inside, d, Js) in lines.items():
        if not inside:
            assert max(abs(J - J0) for J in Js) <= JTOL * abs(J0), name
            _, bound, gd = eg.line_defect(g, d, m, Js, ip)
            assert abs(ip(g, d)) > 100. * bound, (name, abs(ip(g, d)) / gd, bound / gd)
            print("%s %s: |<g,d>| %.1e of |g||d|" % (tag, name, abs(ip(g, d)) / gd))
            seen += 1
    assert seen == 2 * len(pz[0].split()[-1])


def test_poiseuille_a_planted_error_of_1e_8_in_one_coefficient(pz):
    tag, o, X, J0, g, m, ip, lines = pz
    names = [n for n, (inside, _, _) in lines.items() if inside and n != "aligned"]
    for bad_name in names[:4] + names[-2:]:                             # the corners of the first component, the interior of the last
        du = eg.unit(lines[bad_name][1], ip)
        bad = g + 1e-8 * np.sqrt(ip(g, g)) * du
        assert _rel(bad, g) < RTOL
        for name in names:
            defect, bound, gd = eg.line_defect(bad, lines[name][1], m, lines[name][2], ip)
            if name == bad_name:
                assert defect > bound, (name, defect / gd, bound / gd)
            elif abs(ip(du, lines[name][1])) <= 1e-3 * np.sqrt(ip(lines[name][1], lines[name][1])):
                assert defect <= bound, (bad_name, name, defect / gd, bound / gd)      # (needles are not orthogonal under the first-order weights)


# ---- quirk 1: Poiseuille beyond one step ---------------------------------------------------------------------------------------------------
class SolvedDerivatives(PoiseuilleOracle):
    """The Discrete adjoint (s = 0) with the tau solve's own uz, wz, rz in the product adjoints where the reference differentiates the stored
    u, w, rho again: the exact gradient at every N_ITERS.  Test-local on purpose."""

    def forward(self, X):
        self._derivs = None
        return super().forward(X)

    def _nl(self, u, ux, uz, v, vx, vz, rx, rz):
        if self._derivs is None:
            self._derivs = []
        self._derivs.append((uz, vz, rz))                                 # what the products of this step read
        return super()._nl(u, ux, uz, v, vx, vz, rx, rz)

    def adjoint(self, X=None):
        N, dt, ik, W, V = self.N_ITERS, self.dt, 1j * self.k[:, None], self.W, self.V
        Ti, TiA, TA, DzT = self.transformInverse, self.transformInverseAdjoint, self.transformAdjoint, self.Dz
        zero = np.zeros((self.Nxc, self.Nz), dtype=complex)
        ua = -dt * TiA(W * Ti(self.stack[0, :, :, N])) / V
        va = -dt * TiA(W * Ti(self.stack[1, :, :, N])) / V
        ra, uza, vza, rza = zero.copy(), zero.copy(), zero.copy(), zero.copy()
        for idx in range(N - 1, -1, -1):
            ua, va, ra = self._apply_H(self.solve_map, [ua, va, ra, uza, vza, rza], 3)
            uD, vD, rD = self.stack[0, :, :, idx], self.stack[1, :, :, idx], self.stack[2, :, :, idx]
            uzs, vzs, rzs = self._derivs[idx]
            ux, vx, rx, ug, vg = Ti(ik * uD), Ti(ik * vD), Ti(ik * rD), Ti(uD), Ti(vD)
            uzg, vzg, rzg = Ti(uzs), Ti(vzs), Ti(rzs)
            v1, v2, v3 = TA(self.DA * ua), TA(self.DA * va), TA(self.DA * ra)
            adju = TiA(-ux * v1 - vx * v2 - rx * v3)
            adjv = TiA(-uzg * v1 - vzg * v2 - rzg * v3)
            # uz, wz, rz are inputs of the step in their own right: their adjoints go back through the solve (or, at step 0, through Dz)
            ua = ua / dt + adju - ik * TiA(-ug * v1) - dt * TiA(W * ug) / V
            va = va / dt + adjv - ik * TiA(-ug * v2) - dt * TiA(W * vg) / V
            ra = ra / dt - ik * TiA(-ug * v3)
            uza, vza, rza = TiA(-vg * v1), TiA(-vg * v2), TiA(-vg * v3)
        ua = ua + uza @ DzT
        va = va + vza @ DzT
        gu = (V / W) * TA(ua); gv = (V / W) * TA(va)
        return [np.concatenate([np.real(gu).ravel(), np.real(gv).ravel()])]


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("Nx,Nz", [(24, 24), (18, 15)])
def test_poiseuille_beyond_one_step_is_the_references_gradient_not_the_costs(Nx, Nz, n):
    worst = {}
    for cls in (PoiseuilleOracle, SolvedDerivatives):
        o = _pois_oracle(Nx, Nz, n, 0., cls=cls)
        X, J0, g, m, ip, lines = _pois_base(o, "uw", "corners", out_of_band=False)
        shares = []
        for name, (inside, d, Js) in lines.items():
            defect, bound, gd = eg.line_defect(g, d, m, Js, ip)
            assert bound < SHARE * gd
            shares.append((defect / gd, defect / bound))
        worst[cls] = shares
        print("%s %dx%d n=%d: defect %.1e .. %.1e of |g||d|" % (cls.__name__, Nx, Nz, n, min(s[0] for s in shares), max(s[0] for s in shares)))
    assert max(s[1] for s in worst[PoiseuilleOracle]) > 100.               # the reference's adjoint: far outside the bound ...
    assert max(s[0] for s in worst[PoiseuilleOracle]) < 1e-3               # ... and still a gradient to the Taylor tests
    assert max(s[1] for s in worst[SolvedDerivatives]) <= 1.                # the only cause


def test_solved_derivatives_change_nothing_at_one_step():
    o, f = _pois_oracle(24, 24, 1, 0.), _pois_oracle(24, 24, 1, 0., cls=SolvedDerivatives)
    X = eg.white(2 * 24 * 24, SEED, eg.POIS_NORM2, eg.pois_inner_product(24, 24))
    assert o.forward([X]) == f.forward([X])
    assert _rel(f.adjoint([X])[0], o.adjoint([X])[0]) < 1e-13


# ---- quirk 2: SHB23 ------------------------------------------------------------------------------------------------------------------------
class MaskedAdjoint(oshb.SHB23Oracle):
    """The adjoint with the transpose of the de-aliasing mask of nl() applied to r.  Test-local on purpose."""

    def adjoint(self, X=None):
        dt, n_it, W = self.dt, self.N_ITERS, self.W
        p = 2. * oshb.transformInverseAdjoint(W * self.stack[:, n_it]) * dt
        for i in range(n_it):
            r = self.S.T @ p
            b = self.stack[:, n_it - 1 - i]
            rz = r.copy()
            rz[self.N // 2:] = 0.
            p = r / dt + oshb.transformInverseAdjoint((4. * b - 3. * b ** 2) * oshb.transformAdjoint(rz)) + 2. * oshb.transformInverseAdjoint(W * b) * dt
        return [-oshb.transformAdjoint(p) / W]


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("N", [20, 64])
def test_shb23_is_the_references_gradient_not_the_costs(N, n):
    m = eg.degree_half_width("sh23", n)                                    # the same cubic: degree 3^n per step
    theta = np.pi * (np.arange(N) + 0.5) / N
    rs = np.random.RandomState(8)
    worst = {}
    for cls in (oshb.SHB23Oracle, MaskedAdjoint):
        o = cls(N, dt=1e-2, N_ITERS=n)
        X = eg.white(N, SEED, bo.NORM2["shb23"], o.inner)
        o.forward([X])
        g = o.adjoint([X])[0]
        dirs = [("T%d" % k, True, eg.unit(np.cos(k * theta), o.inner)) for k in (0, 1, N // 2 - 1, N // 2, N - 1)]
        dirs += [("white", True, eg.unit(rs.standard_normal(N), o.inner)), ("aligned", True, eg.unit(g, o.inner))]
        shares = []
        for name, (_, d, Js) in _lines(o, X, dirs, m, eg.H, o.inner).items():
            defect, bound, gd = eg.line_defect(g, d, m, Js, o.inner)
            assert bound < SHARE * gd
            shares.append((defect / gd, defect / bound))
        worst[cls] = shares
        print("%s N=%d n=%d: defect %.1e .. %.1e of |g||d|" % (cls.__name__, N, n, min(s[0] for s in shares), max(s[0] for s in shares)))
    assert max(s[1] for s in worst[oshb.SHB23Oracle]) > 100.
    assert max(s[0] for s in worst[oshb.SHB23Oracle]) < 1e-2
    assert max(s[1] for s in worst[MaskedAdjoint]) <= 1.


# ---- the mix-norm cost at one step: which step of the ladder, if any ---------------------------------------------------------------------
def test_mixnorm_cost_at_one_step_has_no_step_that_qualifies():
    """s = 1, one step: rho_1 = S(rho_0 / dt - u dx rho_0 - w rz_0) and dx rho_0 = 0, so J does not depend on u at all (needle and stencil
    both vanish), and it depends on w through rz_0 alone: the analytic derivative of the base profile in the forward solve, Dz rho_0 in the
    adjoint.  A step of the ladder qualifies when the bound is below SHARE / 2 of |g| |d| and every in-band needle is within it on the
    oracle; POIS_MIXNORM_H is the smallest that does, None when none does."""
    ok = {h: True for h in eg.H_LADDER}
    for Nx, Nz in POIS_SIZES[:4]:
        o = _pois_oracle(Nx, Nz, 1, bo.POIS_RI, s=1)
        for h in eg.H_LADDER:
            X, J0, g, m, ip, lines = _pois_base(o, "uw", "corners", h=h, out_of_band=False)
            worst = {"u": (0., 0.), "w": (0., 0.)}
            for name, (_, d, Js) in lines.items():
                if name == "aligned":
                    continue
                defect, bound, gd = eg.line_defect(g, d, m, Js, ip)
                worst[name[0]] = max(worst[name[0]][0], defect / gd), max(worst[name[0]][1], bound / gd)
                if name[0] == "u":
                    gd_, st, _, jscale = eg.blind_defect(g, d, m, Js, ip)
                    assert gd_ <= bound and st <= jscale, (name, gd_ / gd, st / gd)
            for c in "uw":
                print(_PRINT % (("mix-norm %dx%d h=%g %s" % (Nx, Nz, h, c),) + worst[c]))
            ok[h] = ok[h] and all(w[1] < SHARE / 2. and w[0] <= w[1] for w in worst.values())
    qualifying = [h for h in eg.H_LADDER if ok[h]]
    assert eg.POIS_MIXNORM_H == (min(qualifying) if qualifying else None)


# ---- the Hessian identity of SH23 on the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("Npts", [16, 54])
def test_sh23_hessian_is_the_exact_derivative_of_the_gradient(Npts, n):
    o = SH23Oracle(Npts, dt=bo.sh23_dt(Npts), N_ITERS=n)
    ip, m = eg.sh23_inner, eg.degree_half_width("sh23", n)
    X = eg.white(o.G, SEED, eg.SH23_NORM2, ip)
    rs = np.random.RandomState(11)
    Vu, W = eg.unit(rs.standard_normal(o.G), ip), eg.unit(rs.standard_normal(o.G), ip)
    ok = {}
    for h in eg.H_LADDER:
        V = eg.scaled(Vu, X, h, ip)
        _, g, HV = ho.hessvec(o, X, V)
        grads = []
        for Y in eg.line_points(X, V, m):
            o.forward([Y])
            grads.append(o.adjoint([Y], "Discrete")[0])
        defect, bound, hw = eg.hessian_line_defect(W, HV, grads[0::2], grads[1::2], m, ip)
        print("SH23 Hessian %d n=%d h=%g: defect %.1e  bound %.1e  of |HV||W|" % (Npts, n, h, defect / hw, bound / hw))
        assert defect <= bound, (h, defect / hw, bound / hw)
        ok[h] = bound < SHARE * hw
    assert ok[eg.SH23_HESSIAN_H] and eg.SH23_HESSIAN_H == min(h for h in eg.H_LADDER if ok[h])
    assert (GTOL, JTOL) == (1e-11, 1e-12)
