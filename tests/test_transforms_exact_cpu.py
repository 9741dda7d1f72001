"""On the oracle alone (no device): what transform_ops.py and test_transforms_exact_gpu.py rest on.

(a) The closed-form longdouble matrices ARE the reference's maps: the oracle's eight transforms (oracle.shb23.*, PoiseuilleOracle.*) are
    run over the whole table of lengths, shapes and inputs, and their worst defect per family and input kind is printed and held to
    TOL_ULP / 8.  That is where the tolerances of the GPU test come from.
(b) The gap is real and the needle criterion closes it: the exact matrix with ONE entry changed by 1e-11 of its column maximum, applied to
    the random input of the existing direct checks (test_shb23_gpu.py at N = 512, test_poiseuille_gpu.py at 24 x 24), passes their
    rel < 1e-13 / 1e-12 and misses the needle criterion by more than two orders of magnitude (4.5e4 ulp).  So does a Chebyshev matrix whose cosines are taken
    in double of the unreduced argument pi j (2i + 1) / (2N), at the larger Nz of the table.
(c) The tables hold what they are meant to: every radix class of the run-time-length plan, every instantiated length, every tile-remainder
    class of the Poiseuille products.
"""
import os

import numpy as np

from conftest import GOLDEN

import transform_ops as to
from transform_ops import LD, MAPS, TOL_ULP, U


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
def test_oracle_shb23_maps_are_the_closed_form_matrices():
    fns = to.oracle_shb_fns()
    worst = to.Worst()
    for N in to.SHB_LENGTHS:
        for kind, (d, where) in to.shb_worst(N, fns).items():
            assert d <= TOL_ULP["shb23", kind] / 8., (N, kind, d, where)
            worst.see(kind, d, (N,) + where)
    for kind in ("needle", "dense"):
        print("SHB23 oracle, %s inputs: worst defect %.2f ulp at %s (tolerance of the device: %d)" % (kind, *worst[kind], TOL_ULP["shb23", kind]))


def test_oracle_poiseuille_maps_are_the_closed_form_matrices():
    worst = to.Worst()
    for Nx, Nz in to.POIS_SHAPES:
        for kind, (d, where) in to.pois_worst(Nx, Nz, to.oracle_pois_fns(Nx, Nz)).items():
            assert d <= TOL_ULP["pois", kind] / 8., (Nx, Nz, kind, d, where)
            worst.see(kind, d, (Nx, Nz) + where)
    for kind in ("needle", "dense"):
        print("Poiseuille oracle, %s inputs: worst defect %.2f ulp at %s (tolerance of the device: %d)" % (kind, *worst[kind], TOL_ULP["pois", kind]))


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------
def test_shb23_planted_entry_passes_today_and_fails_the_needle_criterion():
    N = 512
    v = np.load(os.path.join(GOLDEN, "shb_helpers.npz"))["v512"]                     # the vector of test_shb23_gpu.py
    for name, M in zip(MAPS, to.shb_matrices(N)):
        for row, col in ((0, 0), (3, 255), (N - 1, 17), (300, N - 1)):
            bad = np.array(M)
            bad[row, col] += LD(1e-11) * np.abs(M[:, col]).max()
            got, ref = (bad @ v.astype(LD)).astype(float), (M @ v.astype(LD)).astype(float)
            whole, needle = rel(got, ref), to.needle_defect(bad[:, col].astype(float), M, col)
            assert 0. < whole < 1e-13, (name, row, col, whole)                       # today's criterion accepts it
            assert needle > 100 * TOL_ULP["shb23", "needle"], (name, row, col, needle)
            assert to.needle_defect(M[:, col].astype(float), M, col) <= 0.5           # and the exact column, rounded, is within half an ulp
    print("SHB23 %d: one entry + 1e-11 of its column: whole-vector rel %.1e, needle defect %.0f ulp" % (N, whole, needle))


def test_poiseuille_planted_entry_passes_today_and_fails_the_needle_criterion():
    Nx, Nz = 24, 24                                                                  # a case of test_poiseuille_gpu.py, and its input
    g = np.random.RandomState(1).standard_normal((Nx, Nz))
    for which in (0, 3):
        re, im, _ = to.pois_expected(Nx, Nz, which, g)
        ref = (re + 1j * im).astype(complex)
        for (n, k), (x, z) in (((0, 0), (0, 0)), ((5, 23), (13, 1)), ((11, 7), (23, 23))):
            nre, nim, scale = to.pois_needle_expected(Nx, Nz, which, x, z)
            delta = float(1e-11 * scale)                                             # entry ((n, k), (x, z)) of the map + 1e-11 of its column
            got = np.array(ref)
            got[n, k] += delta * g[x, z]
            col = (nre + 1j * nim).astype(complex)
            col[n, k] += delta
            assert 0. < rel(got, ref) < 1e-12, (which, n, k, rel(got, ref))
            assert to._pois_defect(col, nre, nim, scale) > 100 * TOL_ULP["pois", "needle"]
            assert to._pois_defect((nre + 1j * nim).astype(complex), nre, nim, scale) <= 0.75


def test_cosines_of_the_unreduced_argument_fail_the_needle_criterion():
    """cos(pi j (2i + 1) / (2N)) in double: the argument reaches j pi and its rounding alone moves the cosine by about 2.7 N ulp.  A transformInverse
    built from it misses the needle criterion, where the existing rel < 1e-12 over a random array never notices; reduced mod 4N in
    integers first, the same double evaluation stays within 4 ulp."""
    for Nz in sorted({Nz for _, Nz in to.POIS_SHAPES} | {192, 384}):
        Bi = to.shb_matrices(Nz)[1]
        i, j = np.arange(Nz)[:, None], np.arange(Nz)[None, :]
        sg = (-1.) ** j
        plain = sg * np.cos(np.pi * j * (2 * i + 1) / (2. * Nz))
        reduced = sg * np.cos(np.pi * ((j * (2 * i + 1)) % (4 * Nz)) / (2. * Nz))
        d_plain = max(to.needle_defect(plain[:, c], Bi, c) for c in range(Nz))
        d_reduced = max(to.needle_defect(reduced[:, c], Bi, c) for c in range(Nz))
        print("Nz = %3d: worst column of Bi in double: unreduced argument %6.1f ulp, reduced %.1f ulp" % (Nz, d_plain, d_reduced))
        assert d_reduced <= 4.
        assert d_plain > Nz                                                          # about 2.7 Nz: above the device's tolerance from Nz = 33 on
        x = np.random.RandomState(1).standard_normal(Nz)
        assert rel(plain @ x, (Bi @ x.astype(LD)).astype(float)) < 1e-12             # ... and today's criterion accepts it


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------
def test_shb23_table_covers_every_plan_class():
    assert set(range(4, 49)) <= set(to.SHB_LENGTHS) and set(to.SHB_INSTANTIATED) <= set(to.SHB_LENGTHS)
    assert all(not to.shb_uses_any_plan(N) for N in to.SHB_INSTANTIATED) and set(to.SHB_ANY_FORCED) <= set(to.SHB_INSTANTIATED)
    runtime = [N for N in to.SHB_LENGTHS if to.shb_uses_any_plan(N)] + to.SHB_ANY_FORCED
    assert set(to.SHB_RUNTIME) <= set(runtime) and min(to.SHB_LENGTHS) == 4 and max(to.SHB_LENGTHS) == 1024
    plans = {N: to.any_plan(N) for N in runtime}
    radices = set().union(*map(set, plans.values()))
    assert {2, 3, 4, 5, 7} <= radices                                                # the butterfly stages
    primes = sorted(r for r in radices if r > 7)                                     # the direct-sum stage
    assert {11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 257, 509, 1021} <= set(primes), primes
    assert any(N % 2 for N in runtime) and {4, 5, 6, 7} <= set(runtime)
    # a direct-sum stage first, last and in the middle of a chain; a chain of one stage and of five
    assert any(p[0] > 7 and len(p) > 1 for p in plans.values()) and any(p[-1] > 7 and len(p) > 1 for p in plans.values())
    assert any(len(p) == 1 for p in plans.values()) and any(len(p) >= 5 for p in plans.values())
    # repeated radices: 7 x 7 x 7, 5 x 5 x 5, 3^5, p x p
    assert plans[343] == [7, 7, 7] and plans[125] == [5, 5, 5] and plans[243] == [3] * 5 and plans[961] == [31, 31]
    for N in to.SHB_LENGTHS:
        nd = to.shb_needles(N)
        assert nd == sorted(set(nd)) and 0 <= nd[0] and nd[-1] == N - 1
        assert len(nd) == N if N <= 64 else {0, 1, 2, 3, N // 2 - 1, N // 2, N // 2 + 1, N - 3, N - 2, N - 1} <= set(nd) and 10 <= len(nd) <= 16


def test_poiseuille_table_covers_every_tile_remainder_class():
    T = to.POIS_TILE
    dims = {s: to.pois_gemm_dims(*s) for s in to.POIS_SHAPES}
    assert any(max(max(d) for d in ds) < T for ds in dims.values())                  # M, N and K below one tile
    for which in range(3):                                                           # M, N, K: a last tile / slice of 1, 2 and 3 elements
        rem = {d[which] % T for ds in dims.values() for d in ds if d[which] > T}
        assert ({1, 2, 3} if which else {2}) <= rem, (which, rem)                    # (M = 2a or Nx is even)
    assert any(Nz % 2 for _, Nz in to.POIS_SHAPES) and any(Nz % 2 == 0 for _, Nz in to.POIS_SHAPES)
    assert any(Nx in to.POIS_XFFT for Nx, _ in to.POIS_SHAPES) and any(Nx not in to.POIS_XFFT for Nx, _ in to.POIS_SHAPES)
    assert all(Nx % 6 == 0 and Nz % 3 == 0 and 12 <= Nx <= 768 and 12 <= Nz <= 384 for Nx, Nz in to.POIS_SHAPES)      # what a context accepts
    for Nx, Nz in to.POIS_SHAPES:
        for coefficient in (False, True):
            nd = to.pois_needles(Nx, Nz, coefficient)
            rows = Nx // 2 if coefficient else Nx
            assert len(nd) == len(set(nd)) and all(0 <= r < rows and 0 <= c < Nz for r, c in nd)
            if Nx * Nz <= 18 * 15:
                assert len(nd) == rows * Nz
            else:
                assert {(r, c) for r in (0, 1, rows // 2, rows - 1) for c in (0, 1, Nz // 2, Nz - 2, Nz - 1)} <= set(nd)
                assert {(r, c) for r in (31, 32, 33) if r < rows for c in (31, 32, 33) if c < Nz} <= set(nd)


def test_defect_measure():
    M = np.array([[1., 2.], [4., -4.]], dtype=LD)
    x = np.array([1., -1.])
    assert to.defect(np.array([-1., 8.]), M, x) == 0.
    assert abs(to.defect(np.array([-1., 8. + 8. * U]), M, x) - 1.) < 1e-12            # |M| |x| = (3, 8): one ulp of 8
    assert abs(to.needle_defect(np.array([2. + 4. * U, -4.]), M, 1) - 1.) < 1e-12    # against the largest entry of the column
    full = to.hermitian_full(4, np.array([[1. + 5j, 2.], [3j, 4.]]))
    assert np.array_equal(full, np.array([[1., 2.], [3j, 4.], [-3j, 4.]]))
