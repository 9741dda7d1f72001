#!/usr/bin/env python3
"""Gram matrix and recombination across the members of a batched KDyn context (smo_gram_dev, smo_combine_dev) against what the parent build
can do and against the plain inner product, device-resident vectors:

    gram_xx   gram_dev(x, x)                 compulsory bytes  B n 8
    gram_xy   gram_dev(x, y)                                  2 B n 8
    combine   combine_dev(C, x)                               2 B n 8
    inner     ONE inner_dev(x, y) call       the bandwidth yardstick, 2 B n 8
    rotated   the same Gram matrix on the PARENT's library (--parent-lib): B inner_dev calls on member-rotated copies of y made with
              smo_vec_axpby (B launches per copy)

and, for a context that never calls the new entry points, milliseconds per gradient (forward + adjoint) of the parent's library and of this
tree in turn (solve_parent, solve_tree).

    python tools/time_kdyn_gram.py --parent-lib /path/to/parent/libsmo.so [--out profiles/r12_kdyn_gram.jsonl]
                                   [--cases 24:16,24:64,128:4] [--solve-cases 24:1000:1,24:1000:64] [--rounds 2] [--seconds 1.0]

Every (case, round, point) runs in a process of its own (a process binds one library), the points alternating inside a round; per point one
warm-up call, whole calls until `--seconds` have passed, then one call with the kernel timing on for the per-launch time of the new timing
classes (the call time includes the launch, the finishing kernel, the copy of the B x B result and the synchronisation; the class time is the
kernel alone).  A child that ends abnormally ends the run.  One JSON line per point; without --parent-lib the parent's points are left out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

NEW = ("smo_gram", "smo_gram_dev", "smo_combine", "smo_combine_dev", "smo_gram_geometry")


def _timed(call, seconds):
    call()
    reps, t0 = 0, time.perf_counter()
    while True:
        call()
        reps += 1
        el = time.perf_counter() - t0
        if el >= seconds:
            return reps, el


def child_block(a):
    from spheremanopt_amd import _capi
    if a.point == "rotated":                        # the parent's library has none of the new entry points to bind
        for name in NEW:
            _capi.SIGNATURES.pop(name, None)
    from spheremanopt_amd import kdyn
    from spheremanopt_amd.devvec import DeviceVector
    N, B = a.npts, a.batch
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(1.0, 1e-3, 1, "Final", batch=B)
    n = ctx.vec_len
    rs = np.random.RandomState(5)
    base = rs.standard_normal(n + B)
    X = DeviceVector.from_numpy(np.concatenate([base[b:b + n] for b in range(B)]))
    Y = DeviceVector.from_numpy(np.concatenate([base[B - b:B - b + n] for b in range(B)]))
    Cm = rs.standard_normal((B, B))
    bytes_ = {"gram_xx": B * n * 8, "gram_xy": 2 * B * n * 8, "combine": 2 * B * n * 8, "inner": 2 * B * n * 8, "rotated": 2 * B * n * 8}[a.point]
    L = _capi.lib()
    if a.point == "gram_xx":
        call = lambda: ctx.gram_dev(X)
    elif a.point == "gram_xy":
        call = lambda: ctx.gram_dev(X, Y)
    elif a.point == "combine":
        O = DeviceVector(B * n)
        call = lambda: ctx.combine_dev(Cm, X, out=O)
    elif a.point == "inner":
        call = lambda: ctx.inner_dev(X, Y)
    else:
        R = DeviceVector(B * n)
        G = np.zeros((B, B))

        def call():
            for s in range(B):
                for b in range(B):
                    _capi._check(L.smo_vec_axpby(0, n, 1.0, C.c_void_p(Y.ptr + 8 * ((b + s) % B) * n), 0.0, None, C.c_void_p(R.ptr + 8 * b * n)))
                v = np.atleast_1d(ctx.inner_dev(X, R))
                G[np.arange(B), (np.arange(B) + s) % B] = v
            return G
    reps, el = _timed(call, a.seconds)
    rec = {"point": a.point, "round": a.round, "npts": N, "G": dom.G, "batch": B, "n": n, "reps": reps, "window_s": el,
           "us_per_call": 1e6 * el / reps, "compulsory_bytes": bytes_, "TBps_per_call": bytes_ / (el / reps) / 1e12,
           "lib": "--parent-lib build" if a.point == "rotated" else "this tree"}
    if a.point == "rotated":                        # the Gram matrix the detour computes, against NumPy (a sanity check of the comparison)
        x, y = X.numpy().reshape(B, n), Y.numpy().reshape(B, n)
        rec["max_rel_err_vs_numpy"] = float(np.abs(call() - x @ y.T / dom.G ** 3).max() / np.abs(x @ y.T / dom.G ** 3).max())
    ctx.timing_enable(True)
    call()
    rec["classes"] = {r["kernel"]: {"launches": r["launches"], "us_per_launch": 1e3 * r["total_ms"] / r["launches"],
                                    "hbm_TBps": r["hbm_bytes_per_launch"] * r["launches"] / (r["total_ms"] * 1e-3) / 1e12}
                      for r in ctx.timing() if r["launches"] and (r["kernel"].startswith("block_") or r["kernel"].startswith("kd_dot"))}
    ctx.timing_enable(False)
    print("RESULT " + json.dumps(rec), flush=True)
    dom.drop_contexts()


def child_solve(a):
    from spheremanopt_amd import _capi
    if a.point == "solve_parent":
        for name in NEW:
            _capi.SIGNATURES.pop(name, None)
    from spheremanopt_amd import kdyn
    from spheremanopt_amd.devvec import DeviceVector, to_device
    N, n_it, B = a.npts, a.steps, a.batch
    dom = kdyn.KDynDomain(N)
    ctx = dom.context(1.0, 1e-3, n_it, "Final", batch=B)
    X = to_device([np.tile(kdyn.synthetic_field(dom.G, 1), B), np.tile(kdyn.synthetic_field(dom.G, 2), B)])
    g = [DeviceVector(B * ctx.vec_len) for _ in range(2)]
    out = {}

    def call():
        out["J"] = ctx.forward_dev(X)
        ctx.adjoint_dev(X, g)
    reps, el = _timed(call, a.seconds)
    rec = {"point": a.point, "round": a.round, "npts": N, "G": dom.G, "n_iters": n_it, "batch": B, "reps": reps, "window_s": el,
           "ms_per_gradient": 1e3 * el / reps / B, "J0": float(np.atleast_1d(out["J"])[0]),
           "lib": "--parent-lib build" if a.point == "solve_parent" else "this tree"}
    print("RESULT " + json.dumps(rec), flush=True)
    dom.drop_contexts()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="24:16,24:64,128:4", help="npts:batch,...")
    ap.add_argument("--solve-cases", default="24:1000:1,24:1000:64", help="npts:steps:batch,... ('' = none)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--child-timeout", type=int, default=240)
    for name, typ in (("point", str), ("npts", int), ("steps", int), ("batch", int), ("round", int)):
        ap.add_argument("--" + name, type=typ, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.point:
        return child_solve(a) if a.point.startswith("solve") else child_block(a)
    out = open(a.out, "w") if a.out else None
    jobs = []
    for case in a.cases.split(","):
        N, B = (int(v) for v in case.split(":"))
        for rnd in range(a.rounds):
            for pt in ["gram_xx", "gram_xy", "combine", "inner"] + (["rotated"] if a.parent_lib else []):
                jobs.append((pt, N, 1, B, rnd))
    for case in [c for c in a.solve_cases.split(",") if c]:
        N, n_it, B = (int(v) for v in case.split(":"))
        for rnd in range(a.rounds):
            for pt in (["solve_parent"] if a.parent_lib else []) + ["solve_tree"]:
                jobs.append((pt, N, n_it, B, rnd))
    for pt, N, n_it, B, rnd in jobs:
        env = dict(os.environ)
        if pt in ("rotated", "solve_parent"):
            env["SMO_LIB"] = os.path.abspath(a.parent_lib)
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--point", pt, "--npts", str(N),
               "--steps", str(n_it), "--batch", str(B), "--round", str(rnd), "--seconds", str(a.seconds)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True)
        lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write("%s npts %d batch %d round %d: exit status %d\n%s\n" % (pt, N, B, rnd, p.returncode, p.stderr[-2000:]))
            return 1                                # nothing more is started on the GPU after a failed point
        print(lines[0], flush=True)
        if out:
            out.write(lines[0] + "\n")
            out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
