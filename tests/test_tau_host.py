"""Host side of the Chebyshev-tau operators of SHB23 and Poiseuille (spheremanopt_amd/csrc/tau_host.hpp) on the CPU: tests/c/tau_host_test.cpp
solves each assembled system with the library's structure-aware LU and with a plain one (equal byte for byte), checks Pre * D == PD,
Tf Ti == I and every entry of Tf and Ti against the closed form in long double, and writes operators that are compared here with the NumPy oracle's builders."""
import os
import subprocess

import numpy as np
import pytest

from oracle import shb23 as osh
from oracle.poiseuille import PoiseuilleCntsOracle, PoiseuilleOracle, solve_map_general

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# relative Frobenius distance to the oracle's operator: 7.2e-14 is the largest measured (SHB23, N = 512); one wrong band entry moves an
# operator by many orders of magnitude more
ORACLE_BOUND = 1e-12


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tau") / "tau_host_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "spheremanopt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "tau_host_test.cpp"), "-o", out], check=True)
    return out


def dumped(exe, tmp_path, dtype, *args):
    path = str(tmp_path / "op.bin")
    r = subprocess.run([exe, "dump", *map(str, args), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(path, dtype=dtype)


def distance(S, ref):
    return float(np.linalg.norm(S - ref) / np.linalg.norm(ref))


def test_structured_lu_equals_plain_lu_and_exact_identities(exe):
    r = subprocess.run([exe, "exact"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout and r.stdout.count("ok ") == 5, r.stdout + r.stderr


@pytest.mark.parametrize("N", [8, 33, 64, 200])
def test_shb23_operator_matches_oracle(exe, tmp_path, N):
    S = dumped(exe, tmp_path, np.float64, "shb", N).reshape(N, N)
    d = distance(S, osh.tau_operator(N, 1e-2))
    print("shb23 N = %d: %.2e" % (N, d))
    assert d <= ORACLE_BOUND


@pytest.mark.parametrize("Nz", [12, 24, 48])
def test_poiseuille_maps_match_oracle(exe, tmp_path, Nz):
    o = PoiseuilleOracle(24, Nz, dt=5e-3)
    for n in (0, 1, 3, 11):
        S = dumped(exe, tmp_path, np.complex128, "solve", Nz, n, 0).reshape(6 * Nz, 3 * Nz)
        M = dumped(exe, tmp_path, np.complex128, "mixnorm", Nz, n).reshape(2 * Nz, Nz)
        ds, dm = distance(S, o.solve_map(n)), distance(M, o.mixnorm_map(n))
        print("poiseuille Nz = %d n = %d: solve %.2e mixnorm %.2e" % (Nz, n, ds, dm))
        assert ds <= ORACLE_BOUND and dm <= ORACLE_BOUND


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("Nz", [12, 24, 48])
def test_poiseuille_ivp_maps_match_oracle(exe, tmp_path, Nz, adjoint):
    h = PoiseuilleCntsOracle(24, Nz, dt=5e-3, N_ITERS=1)
    for n in (0, 1, 3, 11):
        S = dumped(exe, tmp_path, np.complex128, "solve", Nz, n, int(adjoint)).reshape(6 * Nz, 3 * Nz)
        d = distance(S, solve_map_general(h, n, adjoint)[:6 * Nz])
        print("poiseuille IVP Nz = %d n = %d adjoint = %d: %.2e" % (Nz, n, adjoint, d))
        assert d <= ORACLE_BOUND
