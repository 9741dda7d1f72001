"""On the oracle alone (no device): what band_ops.py and test_bands_gpu.py rest on.

(a) The gap is real and the band criterion closes it.  In one of the suite's usual cases per problem (band-limited, pre-smoothed input) a
    defect is planted in the top band of the oracle's own output — the gradient's top band times 1 + 1e-4, the top band of an SH23 snapshot
    set to zero — and the usual whole-vector criterion (rel < 1e-6 / 1e-9) accepts it.  In the white case of the same size band_defects
    rejects 1 + 1e-5 planted in any single band.

(b) The cases are well posed: a condition the oracle must stay within, not a measurement.
    SH23, SHB23: every band of snapshot 1, snapshot n and the gradient's spectral view holds at least FLOOR of its vector.  For SHB23
    Discrete the snapshots are GRID states and the condition is on the stored vector; their Chebyshev spectrum is damped by the step itself
    (1 / (1 + dt k^4) per step: the top quarter of snapshot 4 holds 1e-4 of it at N = 127 and 3e-16 at N = 1024 with dt = 1e-2), so the
    spectral view of those snapshots is judged by the floor rule and its shares are printed.
    Poiseuille: every band of u and w at snapshots 1 .. n - 1, and n when s = 0, holds at least FLOOR.  With s = 1 the Discrete oracle's last
    entry of the stack is not the state: forward() stores (i k psi, psi_z, psi) there, psi the solution of lap psi = rho_n (mixnorm_map), so
    "u" and "w" are derivatives of the inverse Laplacian of a density that is its mean profile plus an O(1e-4) perturbation: mode (k, m)
    carries a factor 1 / (k^2 + m^2) and the x bands above the first hold only the perturbation.  That is damping, so that entry is judged
    by the floor rule.  So are b (mean profile: x bands 1 and 2 hold the perturbation alone), snapshot 0 of the Discrete formulation (its
    top z band is de-aliased: exactly zero) and the gradient components; the under-floor bands of the gradient and of b are counted and
    printed, and together they may be at most one third of all the bands the GPU test judges in the case (3 fields x the snapshots
    0, 1, n - 1, n x 9 + 2 components x 9).
"""
import copy

import numpy as np
import pytest

import band_ops as bo
from band_ops import FLOOR, RTOL, band_defects, band_shares, rel


def _scaled(v, band, factor):
    w = np.array(v)
    w[band] *= factor
    return w


def _rejects_in_every_band(view, bands, tol):
    for b in bands:
        d = band_defects(_scaled(view, b, 1. + 1e-5), view, bands)
        assert max(d) > tol, (b, d)
    assert max(band_defects(view, view, bands)) == 0.


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
def test_sh23_planted_defect_passes_today_and_fails_by_bands():
    from oracle.sh23 import SH23Oracle, synthetic_ic
    Npts, n = 1024, 25                                              # a case of test_sh23_gpu.py
    o = SH23Oracle(Npts, dt=0.02, N_ITERS=n)
    X = synthetic_ic(2 * Npts, 42, 0.0725)
    o.forward([X]); g = o.adjoint([X], "Discrete")[0]
    bands = bo.bands_1d(o.Nc)
    full = np.fft.rfft(g)
    full[bands[-1]] *= 1. + 1e-4
    bad_g = np.fft.irfft(full, n=g.size)
    snap = o.stack[:, n]
    bad_snap = _scaled(snap, bands[-1], 0.)
    print("SH23 %d: shares of the gradient %s, of snapshot %d %s" % (Npts, ["%.1e" % s for s in band_shares(bo.sh23_grad_view(o, g), bands)], n,
                                                                   ["%.1e" % s for s in band_shares(snap, bands)]))
    assert 0. < rel(bad_g, g) < RTOL and rel(bad_snap, snap) < 1e-9 and np.linalg.norm(snap[bands[-1]]) > 0.     # today's criterion accepts both
    # the same defects in the white case of the same size
    r = bo.sh23_ref(Npts)
    for adj in bo.SH23_ADJOINTS:
        view = r[adj]["view"]
        assert band_defects(_scaled(view, r["bands"][-1], 1. + 1e-4), view, r["bands"])[-1] > 10 * RTOL
        _rejects_in_every_band(view, r["bands"], RTOL)
    for i in (1, bo.N_STEPS):
        s = r["snaps"][:, i]
        assert band_defects(_scaled(s, r["bands"][-1], 0.), s, r["bands"])[-1] == 1.
        _rejects_in_every_band(s, r["bands"], bo.SNAP_TOL["sh23"])


def test_shb23_planted_defect_passes_today_and_fails_by_bands():
    from oracle import shb23 as osh
    N, n = 512, 10                                                  # a case of test_parameters_gpu.py / the issue's table
    r = bo.shb23_ref(N)
    o = copy.copy(r["o"])                                            # same dt, so the same tau operator
    o.N_ITERS = n
    X = osh.synthetic_ic(o, 42, 0.0019)
    o.forward([X]); g = o.adjoint([X])[0]
    bands = r["bands"]
    c = osh.transform(g)
    print("SHB23 %d: shares of the gradient %s" % (N, ["%.1e" % s for s in band_shares(c, bands)]))
    bad_g = osh.transformInverse(_scaled(c, bands[-1], 1. + 1e-4))
    assert 0. < rel(bad_g, g) < RTOL
    assert rel(osh.transformInverse(c), g) < 1e-13                  # (the round trip itself is exact to rounding)
    assert band_defects(_scaled(r["view"], bands[-1], 1. + 1e-4), r["view"], bands)[-1] > 10 * RTOL
    _rejects_in_every_band(r["view"], bands, RTOL)
    for i in (1, bo.N_STEPS):
        _rejects_in_every_band(r["snaps"][:, i], bands, bo.SNAP_TOL["shb23"])


def test_poiseuille_planted_defect_passes_today_and_fails_by_bands():
    from oracle.poiseuille import PoiseuilleOracle, synthetic_ic
    Nx, Nz, n, s = 96, 48, 4, 0                                     # a case of test_poiseuille_gpu.py
    o = PoiseuilleOracle(Nx, Nz, dt=5e-3, N_ITERS=n, s=s, delta=0.3)
    X = synthetic_ic(o, 42)
    o.forward([X]); g = o.adjoint([X])[0]
    gu, gw = o.split(g)
    c = o.transform(gu)                                              # (Nxc, Nz): wavenumbers 0..kmax, -kmax..-1
    e = np.linspace(0, o.ax, 4).astype(int)
    top = (np.abs(o.n) >= e[2])[:, None]
    print("Poiseuille %d x %d: x-band shares of g_u %s" % (Nx, Nz, ["%.1e" % np.sqrt(sum(v ** 2 for v in band_shares(c[:o.ax], bo.bands_2d(o.ax, Nz))[3 * i:3 * i + 3]))
                                                                    for i in range(3)]))
    bad_gu = np.real(o.transformInverse(np.where(top, (1. + 1e-4) * c, c)))
    bad = np.concatenate([bad_gu.ravel(), gw.ravel()])
    assert 0. < rel(bad, g) < RTOL and rel(np.real(o.transformInverse(c)), gu) < 1e-12
    r = bo.pois_ref(Nx, Nz, 2, s)                                   # the white case of the same size
    bands = r["bands_grad"]
    for view in r["views"]:
        for xb in range(3):                                          # a whole x band, as above, and then every rectangle
            w = np.array(view)
            w[bands[3 * xb][0]] *= 1. + 1e-4
            assert max(band_defects(w, view, bands)[3 * xb:3 * xb + 3]) > 10 * RTOL
        _rejects_in_every_band(view, bands, RTOL)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------
SH23_ALL = sorted({(N, bo.N_STEPS, bo.SEED) for N in bo.SH23_SIZES + [bo.SH23_ANY_SIZE]}
                  | {(N, bo.N_STEPS, sd) for N in bo.SH23_BATCH_SIZES for sd in bo.BATCH_SEEDS}
                  | {(bo.SH23_HORIZONS[0], nb, sd) for nb, sd in zip(bo.SH23_HORIZONS[1], bo.BATCH_SEEDS)})


@pytest.mark.parametrize("Npts,n,seed", SH23_ALL)
def test_sh23_cases_are_well_posed(Npts, n, seed):
    r = bo.sh23_ref(Npts, n, seed)
    assert abs(r["o"].inner(r["X"], r["X"]) - bo.NORM2["sh23"]) < 1e-15
    kmax = 2. * np.pi * (Npts // 2) / bo.SH23_L
    damping = r["dt"] * (1. - kmax ** 2) ** 2                        # the top mode is divided by about 1 + this per step
    assert r["dt"] == 0.1 and damping <= 10. or 0.1 < damping <= 1.0000001, (r["dt"], damping)
    sh = {"snapshot 1": band_shares(r["snaps"][:, 1], r["bands"]), "snapshot n": band_shares(r["snaps"][:, n], r["bands"])}
    for adj in bo.SH23_ADJOINTS:
        sh[adj] = band_shares(r[adj]["view"], r["bands"])
    print("SH23 %d n %d dt %g: smallest share %.2e" % (Npts, n, r["dt"], min(min(v) for v in sh.values())))
    for k, v in sh.items():
        assert min(v) >= FLOOR, (k, v)


SHB23_ALL = [(N, False, bo.SEED) for N in bo.SHB23_SIZES] + [(N, False, sd) for N in bo.SHB23_BATCH_SIZES for sd in bo.BATCH_SEEDS[1:]] + \
            [(N, True, bo.SEED) for N in bo.SHB23C_SIZES] + [(N, True, sd) for N in bo.SHB23C_BATCH_SIZES for sd in bo.BATCH_SEEDS[1:]]


@pytest.mark.parametrize("N,continuous,seed", SHB23_ALL)
def test_shb23_cases_are_well_posed(N, continuous, seed):
    n = bo.N_STEPS
    r = bo.shb23_ref(N, continuous, n, seed)
    assert abs(r["o"].inner(r["X"], r["X"]) - bo.NORM2["shb23"]) < 1e-15
    sh = {"snapshot 1": band_shares(r["snaps"][:, 1], r["bands"]), "snapshot n": band_shares(r["snaps"][:, n], r["bands"]),
          "gradient": band_shares(r["view"], r["bands"])}
    spec = [min(band_shares(bo.shb23_snap_view(r["snaps"][:, i], continuous), r["bands"])) for i in (1, n)]
    print("SHB23 %s %d dt %g: smallest share %.2e; of the snapshots' spectra %.1e (1), %.1e (n)"
          % ("Continuous" if continuous else "Discrete", N, r["dt"], min(min(v) for v in sh.values()), spec[0], spec[1]))
    for k, v in sh.items():
        assert min(v) >= FLOOR, (k, v)


def pois_band_census(r, n, s, continuous):
    """(smallest share among the u, w bands under the condition, number of under-floor bands of the gradient and of b, number of bands the
    GPU test judges)."""
    idx = sorted({0, 1, n - 1, n})
    keep = r["xkeep"]
    cond = [min(band_shares(r["snaps"][(f, i)][:keep], r["bands_snap"])) for f in (0, 1) for i in range(1, n + (1 if s == 0 or continuous else 0))]
    under_b = sum(x < FLOOR for i in idx for x in band_shares(r["snaps"][(2, i)][:keep], r["bands_snap"]))
    under_g = sum(x < FLOOR for v in r["views"] for x in band_shares(v, r["bands_grad"]))
    return min(cond), under_g, under_b, 27 * len(idx) + 18


POIS_ALL = [(Nx, Nz, n, s, False, bo.SEED) for Nx, Nz, n in bo.POIS_SIZES for s in (0, 1)] + \
           [bo.POIS_VARIANT_SIZE + (s, False, sd) for s in (0, 1) for sd in bo.BATCH_SEEDS[1:]] + \
           [(Nx, Nz, n, s, True, bo.SEED) for Nx, Nz, n in bo.POISC_SIZES for s in (0, 1)]


@pytest.mark.parametrize("Nx,Nz,n,s,continuous,seed", POIS_ALL)
def test_poiseuille_cases_are_well_posed(Nx, Nz, n, s, continuous, seed):
    r = bo.pois_ref(Nx, Nz, n, s, continuous, seed)
    o = r["o"]
    assert abs(o.inner(r["X"], r["X"]) - bo.NORM2["pois"]) < 1e-15
    assert r["dt"] == bo.POIS_LADDER[0]                              # the largest of the ladder: nothing larger to rule out
    smallest, under_g, under_b, judged = pois_band_census(r, n, s, continuous)
    print("Poiseuille %s %d x %d n %d s %d: smallest u, w share %.2e; under the floor: %d gradient bands, %d b bands of %d judged"
          % ("Continuous" if continuous else "Discrete", Nx, Nz, n, s, smallest, under_g, under_b, judged))
    assert smallest >= FLOOR
    assert 3 * (under_g + under_b) <= judged
    if not continuous:                                               # the de-aliased rows: exactly zero in every snapshot
        for k, v in r["snaps"].items():
            assert v.shape == (o.ax, Nz) and not np.any(v[o.a:]), k
        if s == 1:                                                   # the last entry is the mix-norm potential, not the state (see above)
            last = [min(band_shares(r["snaps"][(f, n)][:o.a], r["bands_snap"])) for f in (0, 1)]
            before = [min(band_shares(r["snaps"][(f, n - 1)][:o.a], r["bands_snap"])) for f in (0, 1)]
            print("    last entry (i k psi, psi_z): smallest shares %.1e %.1e, the state before it %.1e %.1e" % (*last, *before))
            assert np.array_equal(o.stack[0, :, :, n], 1j * o.k[:, None] * o.stack[2, :, :, n])       # the u slot is i k psi of the b slot


def test_band_helpers():
    assert [b[0] for b in bo.bands_1d(11)] == [slice(0, 2), slice(2, 5), slice(5, 8), slice(8, 11)]
    rect = bo.bands_2d(7, 9)
    assert len(rect) == 9 and rect[0] == (slice(0, 2), slice(0, 3)) and rect[-1] == (slice(4, 7), slice(6, 9))
    cover = np.zeros((7, 9), dtype=int)
    for b in rect:
        cover[b] += 1
    assert np.all(cover == 1)
    ref = np.array([1., 0., 0., 1e-6])
    got = ref + np.array([0., 0., 0., 1e-9])
    d = band_defects(got, ref, bo.bands_1d(4), 1e-3)
    assert d[:3] == [0., 0., 0.] and abs(d[3] - 1e-9 / 1e-3) < 1e-12          # a band under the floor: against floor x the whole vector
    assert abs(band_defects(got, ref, bo.bands_1d(4), 1e-9)[3] - 1e-3) < 1e-9  # one above it: against its own norm
    for kind, shape, size in (("sh23", 16, 32), ("shb23", 20, 20), ("shb23c", 32, 64), ("pois", (24, 24), 1152), ("poisc", (16, 16), 1152)):
        x = bo.white_input(kind, shape, 5)
        assert x.shape == (size,) and not x.flags.writeable
        assert np.array_equal(x, bo.white_input(kind, shape, 5)) and not np.array_equal(x, bo.white_input(kind, shape, 6))
        assert abs(bo.make_oracle(kind, shape, 1).inner(x, x) - bo.NORM2[kind.rstrip("c")]) < 1e-15
