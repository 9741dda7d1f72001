"""Gram matrix and recombination across the members of a batched context (smo_gram*, smo_combine*), the parts that need no GPU: the four
entry points are declared, exported and bound; the Python front end refuses bad arguments before the library is touched; the subspace
iteration built on them finds the leading singular values of an explicit matrix; and the chunk / tile index arithmetic the kernels share with
the host (csrc/blockops_tiles.hpp) owns every (member, element) pair exactly once."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from spheremanopt_amd import _capi, subspace

_DECLS = (("smo_gram", "int smo_gram(smo_ctx*, const double* x, const double* y, double* out)"),
          ("smo_gram_dev", "int smo_gram_dev(smo_ctx*, const double* x_dev, const double* y_dev, double* out_host)"),
          ("smo_combine", "int smo_combine(smo_ctx*, const double* C, const double* x, double* out)"),
          ("smo_combine_dev", "int smo_combine_dev(smo_ctx*, const double* C_host, const double* x_dev, double* out_dev)"))


def _types(params):
    """Parameter list -> the types alone ('const double*', ...), whatever the names."""
    out = []
    for p in params.split(","):
        p = re.sub(r"\s+", " ", p.strip()).replace(" *", "*")
        m = re.match(r"^(.*\*)\s*\w*$", p)
        out.append(m.group(1).strip() if m else p)
    return out


def test_entry_points_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smo.h")).read(), flags=re.S)
    for name, want in _DECLS:
        m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % name, hdr)
        assert m, "include/smo.h does not declare %s" % name
        assert _types(m.group(1)) == _types(re.search(r"\((.*)\)", want).group(1)), (name, m.group(1))
        assert name in _capi.SIGNATURES and name in _capi.EXPORTS
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is _capi.C.c_int and len(argtypes) == 4
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    for name, _ in _DECLS:
        assert hasattr(_capi.lib(), name)


class _Vec:
    """Describes itself like a DeviceVector; holds no memory."""

    def __init__(self, n, device=0):
        self.n, self.device, self.ptr = n, device, 4096

    def numpy(self):
        raise AssertionError("a device vector was downloaded")


def _bare_context(cls=_capi.Context, batch=3, vec_len=10):
    ctx = cls.__new__(cls)
    ctx.batch, ctx.vec_len, ctx.ncomp, ctx.ngrad, ctx._h = batch, vec_len, 1, 1, None
    ctx.cfg = _capi.smo_config(device=0)
    return ctx


def test_front_end_refuses_before_the_library_is_touched(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_capi, "lib", no_lib)
    ctx = _bare_context()
    x, good = _Vec(30), np.eye(3)
    for bad in (np.eye(2), np.zeros((3, 4)), np.zeros(9), np.zeros((1, 3, 3))):
        with pytest.raises(ValueError, match="shape"):
            ctx.combine_dev(bad, x)
        with pytest.raises(ValueError, match="shape"):
            ctx.combine(bad, np.zeros(30))
    with pytest.raises(ValueError, match="29 entries"):
        ctx.combine_dev(good, _Vec(29))
    with pytest.raises(ValueError, match="29 entries"):
        ctx.combine_dev(good, x, out=_Vec(29))
    with pytest.raises(ValueError, match="29 entries"):
        ctx.gram_dev(_Vec(29))
    with pytest.raises(ValueError, match="31 entries"):
        ctx.gram_dev(x, _Vec(31))
    with pytest.raises(ValueError, match="device 1"):
        ctx.gram_dev(x, _Vec(30, device=1))
    with pytest.raises(ValueError, match="29 entries"):
        ctx.gram(np.zeros(29))
    with pytest.raises(ValueError, match="31 entries"):
        ctx.combine(good, np.zeros(31))
    with pytest.raises(ValueError, match="out is x"):
        ctx.combine_dev(good, x, out=x)
    with pytest.raises(TypeError):
        ctx.gram_any(x, np.zeros(30))
    multi = _bare_context(_capi.MultiContext, batch=1)
    multi.devices = [0, 0]
    for call in (lambda: multi.gram(np.zeros(10)), lambda: multi.gram_dev(_Vec(10)), lambda: multi.combine(np.eye(1), np.zeros(10)),
                 lambda: multi.combine_dev(np.eye(1), _Vec(10))):
        with pytest.raises(ValueError, match="multi-device"):
            call()


# ---- subspace iteration on an explicit matrix ---------------------------------------------------------------------------------------------
def _explicit_problem():
    rs = np.random.RandomState(12)
    Q1, _ = np.linalg.qr(rs.standard_normal((40, 40)))
    Q2, _ = np.linalg.qr(rs.standard_normal((40, 40)))
    sigma = 2. ** -np.arange(40)
    A = Q1 @ np.diag(sigma) @ Q2.T
    return A, sigma, rs.standard_normal((4, 40))


def test_subspace_iteration_finds_the_leading_singular_values():
    """A = Q1 diag(2^0 .. 2^-39) Q2^T, k = 4, 30 sweeps: the convergence factor (sigma_5 / sigma_4)^(2 * 30) = 2^-60 is below rounding, so the
    Ritz values are sigma_1^2 .. sigma_4^2 to 1e-12 relative and the seeds are orthonormal to 1e-12."""
    A, sigma, X0 = _explicit_problem()
    be = subspace.NumpyBackend(lambda x: A @ x, lambda y: A.T @ y)
    ritz, X, history = subspace.leading_seeds(be, X0, 30)
    err = np.abs(ritz - sigma[:4] ** 2) / sigma[:4] ** 2
    orth = np.abs(X @ X.T - np.eye(4)).max()
    print("Ritz relative errors", err, " |X X^T - I| =", orth)
    assert history.shape == (30, 4) and np.array_equal(history[-1], ritz)
    assert np.all(np.diff(ritz) < 0)                                       # descending
    assert np.all(err <= 1e-12), err
    assert orth <= 1e-12, orth


def test_orthonormalise_returns_the_factor_and_refuses_a_rank_deficient_block():
    A, _, X0 = _explicit_problem()
    be = subspace.NumpyBackend(lambda x: A @ x, lambda y: A.T @ y)
    Q, R = subspace.orthonormalise(be, X0)
    assert np.abs(Q @ Q.T - np.eye(4)).max() <= 1e-13
    assert np.allclose(np.tril(R, -1), 0.) and np.abs(be.combine(Q, R) - X0).max() <= 1e-13 * np.abs(X0).max()
    X0[2] = X0[0]                                                          # two equal members
    with pytest.raises(np.linalg.LinAlgError, match="pass 1"):
        subspace.orthonormalise(be, X0)
    with pytest.raises(np.linalg.LinAlgError, match="pass 1"):
        subspace.leading_seeds(be, np.stack([X0[0], X0[1], X0[1], X0[3]]), 3)


# ---- the kernels' index arithmetic, in a program of its own ----------------------------------------------------------------------------------
def _compile(out, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "spheremanopt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "blockops_tiles_test.cpp"), "-o", out], capture_output=True, text=True)


def test_every_member_element_pair_is_owned_once_and_padding_is_flagged(tmp_path):
    """tests/c/blockops_tiles_test.cpp walks block_gram's loader for n in 1..70, 2187, 5184, 10125 and B in 1, 2, 3, 16, 17, 33, 64, 65 (and
    G = 36 with B = 3, 17, 256).  Built with the address and undefined-behaviour sanitizers where the host compiler has them."""
    out = str(tmp_path / "blockops_tiles_test")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0:                                                  # a compiler without the sanitizer runtimes
        print("sanitizers unavailable:", r.stderr[-300:])
        r = _compile(out, [])
    assert r.returncode == 0, r.stderr
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout[-600:])
    assert r.returncode == 0 and "FAIL" not in r.stdout and "ok 587 cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
