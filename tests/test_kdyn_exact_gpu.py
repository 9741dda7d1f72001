"""Oracle-free EXACT checks of both KDyn gradients and of every mode of the time step (tests/exact_ops.py states the two identities,
test_kdyn_exact_cpu.py pins them on the CPU oracle and shows that they reject a 1e-8 error in one Fourier coefficient).

A.  Needles.  <g, d> = sum_j w_j (J(+j d) - J(-j d)) with the stencil weights that are exact for the degree of J along the line (1 in B0,
    2n in U), Discrete adjoint, d a unit plane wave a cos(k.x + phi) with a perp k on the corners, edges and faces of the retained cube
    and inside it, and d = gU / |gU|.  Bound: JTOL = 1e-12 on every J the stencil reads plus GTOL = 1e-11 on |g| |d| (the form and the
    figures of test_symmetry_gpu.test_kdyn_cost_is_a_quadratic_form_in_B0); the bound itself must stay below 1e-8 |g| |d|.
B.  Uniform flow.  Snapshot i = the i-fold application of the per-mode 3 x 3 step, evaluated in longdouble, to the device's own snapshot 0,
    element by element over every retained mode.  Bound: 32 times the oracle's own defect against that closed form (9.6e-16 of max |S_0|
    -> UNIFORM_TOL = 3.2e-14).

Largest figures observed on an MI355X (a run with -s prints the table at its end).  Needles: the defect as a share of its bound, and the
bound as a share of |g| |d| (which must stay below 1e-8):
                                        gB needle   gU needle   gU aligned      bound gB   bound gU
    Npts 6 .. 40, one batch of 64:        4.9e-5      2.0e-4      2.5e-4         1.2e-11    1.3e-10
    Npts 44 .. 128:                       3.2e-4      9.2e-4      7.9e-4         1.3e-11    3.1e-10
    Npts 192, 256:                        3.2e-4      1.3e-3      6.7e-4         1.3e-11    2.4e-10
    n = 3, ckpt = 2:                      1.3e-5      7.7e-5      1.1e-5         1.1e-11    7.5e-11
    SMO_KD_ANY=1:                         1.6e-5      9.9e-5      3.4e-5         1.1e-11    4.7e-11
    captured-graph replay:                9.3e-6      5.7e-5      5.3e-5         1.1e-11    6.0e-11
    devices [0, 0]:                       6.0e-6      1.1e-4      2.6e-5         1.1e-11    4.7e-11
    frozen_U:                             1.3e-5                                 1.1e-11
so the largest defect seen is 3e-13 of |g| |d| (gU, Npts 192 / 256).
Uniform flow: max |delta| / max |S_0| = 6.5e-16 over the eight sizes (the oracle: 9.6e-16; the bound: 3.2e-14); with ckpt = 2,
|J + energy| = 2.4e-16 |J|.
"""
import numpy as np
import pytest

import test_symmetry_gpu as sym
from exact_ops import (GTOL, JTOL, SHARE, UNIFORM_FLOW, UNIFORM_TOL, boundary_needles, few_needles, inner, needle_defect,
                       needle_wavenumbers, stencil_weights, uniform_flow_steps, unit_needle, wavenumbers)
from spheremanopt_amd import kdyn
from spheremanopt_amd.devvec import DeviceVector
from symmetry_ops import kd_cheap_field

pytestmark = pytest.mark.gpu
assert (JTOL, GTOL) == (sym.JTOL, sym.GTOL)
RM = sym.RM
BATCHED_UP_TO = 40                        # Npts: up to here every perturbed solve of a size is a member of ONE batched call

_WORST = {}


def _note(family, share):
    _WORST[family] = max(_WORST.get(family, 0.), float(share))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(_WORST):
        print("\nlargest  %-44s %.2e" % (fam, _WORST[fam]), end="")
    print()


# ---- A: needles ----------------------------------------------------------------------------------------------------------------------
def _jobs(which, n, d):
    """The (B0 or U, multiple of d) pairs one direction needs: +-1 for gB, +-1 .. +-n for gU."""
    return [(which, s * j, d) for j in range(1, (n if which == "U" else 1) + 1) for s in (1, -1)]


def _solve_jobs(dom, ctx1, cost, n, B, U, jobs, how):
    """J of every job.  how = "batch": all of them as members of one batched context, one call; "host": one call each on the base context
    with host vectors; "device": the same with vectors that stay in HBM (B0, U and each direction cross PCIe once)."""
    G = dom.G
    if how == "batch":
        ctx = dom.context(RM, sym._kd_dt(G), n, cost, batch=len(jobs))
        Bs = np.concatenate([B + t * d if which == "B" else B for which, t, d in jobs])
        Us = np.concatenate([U + t * d if which == "U" else U for which, t, d in jobs])
        return list(ctx.forward([Bs, Us]))
    if how == "host":
        return [ctx1.forward([B + t * d, U] if which == "B" else [B, U + t * d]) for which, t, d in jobs]
    Bd, Ud, out, up = DeviceVector.from_numpy(B), DeviceVector.from_numpy(U), [], (None, None)
    for which, t, d in jobs:
        if up[0] is not d:
            up = (d, DeviceVector.from_numpy(d))
        out.append(ctx1.forward_any([Bd + t * up[1], Ud] if which == "B" else [Bd, Ud + t * up[1]]))
    return out


def _check_needles(N, ks, how, family, n=2, cost=None, frozen=False, inputs=None, count_replays=False, **dom_kw):
    dom = kdyn.KDynDomain(N, **dom_kw)
    G = dom.G
    cost = cost or sym._COMBO[N][0]
    B, U = inputs or sym._kd_inputs(G)
    ctx1 = dom.context(RM, sym._kd_dt(G), n, cost, frozen_U=frozen)
    ctx1.forward([B, U])
    g = dict(zip("BU", ctx1.adjoint(None, "Discrete")))                    # (a frozen-velocity context fills dJ/dB0 alone)
    rs = np.random.RandomState(3)
    dirs = [("needle", unit_needle(G, k, rs)) for k in ks]
    plan = [(which, kind, d) for kind, d in dirs for which in sorted(g)]
    if "U" in g:
        plan.append(("U", "aligned", g["U"] / np.sqrt(inner(g["U"], g["U"], G))))
    jobs = [job for which, kind, d in plan for job in _jobs(which, n, d)]
    Js = _solve_jobs(dom, ctx1, cost, n, B, U, jobs, how)
    failures = []
    for which, kind, d in plan:
        m = n if which == "U" else 1
        mine, Js = Js[:2 * m], Js[2 * m:]
        defect, bound, gd = needle_defect(g[which], d, stencil_weights(m), mine[0::2], mine[1::2], G)
        _note("%s g%s %s: defect / bound" % (family, which, kind), defect / bound)
        _note("%s g%s: bound / (|g| |d|)" % (family, which), bound / gd)
        if not (defect <= bound and bound < SHARE * gd):
            failures.append((which, kind, defect / gd, bound / gd))
    info = ctx1.get(2) if count_replays else None             # smo_get key 2: graph replays of the base context
    dom.drop_contexts()
    assert not failures, failures
    return info


@pytest.mark.parametrize("N", sym._SMALL)
def test_gradient_needles(N):
    """Every tuned size up to 128 and the run-time-length sizes: ten needles (three above Npts 40) and the aligned direction, for dJ/dB0
    and dJ/dU; the two costs alternate over the sizes."""
    kmax = (N - 1) // 2
    if N <= BATCHED_UP_TO:
        _check_needles(N, needle_wavenumbers(kmax), "batch", "needles Npts <= 40")
    else:
        _check_needles(N, few_needles(kmax), "device", "needles Npts 44..128")


@pytest.mark.parametrize("N", [192, 256])
def test_gradient_needles_large_sizes(N):
    """G = 288 and 384: the two needles on the truncation boundary and the aligned direction."""
    G = 3 * N // 2
    inputs = kd_cheap_field(G, 9), kd_cheap_field(G, 10, mean=0.)
    _check_needles(N, boundary_needles((N - 1) // 2), "device", "needles Npts 192, 256", inputs=inputs)


def test_gradient_needles_three_steps_across_a_window():
    """n = 3 (stencil +-1 .. +-3) with ckpt = 2: the running sum of omega x B_f crosses a checkpoint-window boundary."""
    _check_needles(16, needle_wavenumbers(7), "host", "needles n = 3, ckpt = 2", n=3, cost="Integrated", ckpt=2)


def test_gradient_needles_runtime_length_kernels(monkeypatch):
    monkeypatch.setenv("SMO_KD_ANY", "1")
    _check_needles(16, needle_wavenumbers(7), "batch", "needles SMO_KD_ANY=1", cost="Final")


def test_gradient_needles_captured_graph_replay():
    replays = _check_needles(24, few_needles(11), "host", "needles graph replay", cost="Integrated", count_replays=True)
    assert replays >= 3 * (2 + 4) + 4, replays                      # every perturbed solve replayed the captured forward graph


def test_gradient_needles_two_slabs_in_one_process():
    _check_needles(16, few_needles(7), "host", "needles devices [0, 0]", cost="Final", devices=[0, 0])


def test_gradient_needles_frozen_velocity():
    """dJ/dB0 of a frozen_U context (its adjoint x pass forms omega x U alone)."""
    _check_needles(16, needle_wavenumbers(7), "host", "needles frozen_U", cost="Integrated", frozen=True)


# ---- B: uniform flow -----------------------------------------------------------------------------------------------------------------
def _uniform_inputs(G):
    return kd_cheap_field(G, 9), np.repeat(np.array(UNIFORM_FLOW), G ** 3)


@pytest.mark.parametrize("N", [8, 10, 16, 22, 28, 40, 64, 128])      # radix 2, 3, 5, 7, odd G, run-time length, the bench grid
def test_uniform_flow_every_mode(N):
    n, dt = 5, 1e-2
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(RM, dt, n, "Final")
    ctx.forward(_uniform_inputs(dom.G))
    S = [ctx.snapshot(i).view(np.complex128).reshape(3, dom.a, dom.m, dom.m) for i in range(n + 1)]
    dom.drop_contexts()
    scale = float(np.abs(S[0]).max())
    worst = 0.
    for i, E in enumerate(uniform_flow_steps(S[0], wavenumbers(N), UNIFORM_FLOW, RM, dt, n), 1):
        worst = max(worst, float(np.abs(S[i] - E).max()) / scale)
    _note("uniform flow: max |delta| / max |S_0|", worst)
    assert worst <= UNIFORM_TOL, worst


def test_uniform_flow_with_checkpoint_windows():
    """ckpt = 2, n = 5: the snapshots are not readable under windows, so J(Final) is compared with the spectral energy of the closed-form
    last snapshot (the weights of test_size_independent_properties), started from snapshot 0 of a keep-all context."""
    N, n, dt = 16, 5, 1e-2
    dom = kdyn.KDynDomain(N)
    B, U = _uniform_inputs(dom.G)
    ctx = dom.context(RM, dt, 1, "Final")
    ctx.forward([B, U])
    S0 = ctx.snapshot(0).view(np.complex128).reshape(3, dom.a, dom.m, dom.m)
    dom.drop_contexts()
    K = wavenumbers(N)
    last = list(uniform_flow_steps(S0, K, UNIFORM_FLOW, RM, dt, n))[-1]
    energy = float((np.where(K[0] == 0, 1., 2.) * np.abs(last) ** 2).sum())
    dom = kdyn.KDynDomain(N, ckpt=2)
    J = dom.context(RM, dt, n, "Final").forward([B, U])
    dom.drop_contexts()
    _note("uniform flow, ckpt = 2: |J + energy| / |J|", abs(J + energy) / abs(J))
    assert abs(J + energy) <= JTOL * abs(J), (J, energy)
