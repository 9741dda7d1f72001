#!/usr/bin/env python3
"""KDyn with a frozen velocity (smo_create_frozen_u) against the full-gradient context: milliseconds per gradient (forward + adjoint,
device-resident vectors) of

    parent   the full context of ANOTHER build of the library (--parent-lib: libsmo.so of the parent commit)
    full     the full context of this tree
    frozen   the frozen-velocity context, keep_states = 1
    nostack  the frozen-velocity context, keep_states = 0 (Final cost: no snapshot stack)

    python tools/time_kdyn_frozen.py --parent-lib /path/to/parent/libsmo.so [--out profiles/r10_kdyn_frozen_u.jsonl]
                                     [--cases 128:200:1,24:1000:1,24:1000:64,256:100:1] [--rounds 2] [--seconds 1.0]
                                     [--variants parent,full,frozen,nostack]        which ones, in the order they take turns

Every (case, round, variant) runs in a process of its own (a process binds one library), the four variants alternating inside a round, so
that a drift of the machine lands on all of them (measuring guide: interleave, repeat, report every round).  Per point: one warm-up
gradient (graph capture at G <= 36), whole gradients until `--seconds` have passed, then one gradient with the kernel timing on for the
per-launch time and the achieved HBM rate (compulsory bytes) of the x-pass classes.  A child that ends abnormally ends the run.
One JSON line per point; without --parent-lib the parent variant is left out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def free_hbm():
    try:
        fn = C.CDLL(None).hipMemGetInfo
        a, b = C.c_size_t(), C.c_size_t()
        return int(a.value) if fn(C.byref(a), C.byref(b)) == 0 else None
    except (AttributeError, OSError):
        return None


def child(a):
    from spheremanopt_amd import _capi
    if a.variant == "parent":                       # the parent's library has no smo_create_frozen_u to bind
        _capi.SIGNATURES.pop("smo_create_frozen_u", None)
    from spheremanopt_amd import kdyn
    from spheremanopt_amd.devvec import DeviceVector, to_device
    N, n, B = a.npts, a.steps, a.batch
    f = np.load(a.fields)
    dom = kdyn.KDynDomain(N)
    frozen = a.variant in ("frozen", "nostack")
    ctx = dom.context(1.0, 1e-3, n, "Final", batch=B, **({"frozen_U": True, "keep_states": a.variant == "frozen"} if frozen else {}))
    X = to_device([np.tile(f["B"], B), np.tile(f["U"], B)])
    g = [DeviceVector(B * ctx.vec_len) for _ in range(1 if frozen else 2)]
    t0 = time.perf_counter()
    ctx.forward_dev(X); ctx.adjoint_dev(X, g)
    first = time.perf_counter() - t0
    free = free_hbm()
    reps, t0 = 0, time.perf_counter()
    while True:
        J = ctx.forward_dev(X); ctx.adjoint_dev(X, g)
        reps += 1
        el = time.perf_counter() - t0
        if el >= a.seconds:
            break
    rec = {"variant": a.variant, "round": a.round, "npts": N, "G": dom.G, "n_iters": n, "batch": B, "reps": reps, "window_s": el,
           "first_call_ms": 1e3 * first, "ms_per_gradient": 1e3 * el / reps / B, "ms_per_call_pair": 1e3 * el / reps,
           "stack_bytes": ctx.stack_bytes, "ty_stack_bytes": ctx.get(1), "ckpt": ctx.get(0), "graph_replays": ctx.get(2),
           "free_hbm_bytes": free, "J0": float(np.atleast_1d(J)[0]), "lib": "--parent-lib build" if a.variant == "parent" else "this tree"}
    ctx.timing_enable(True)
    ctx.forward_dev(X); ctx.adjoint_dev(X, g)
    rec["x_pass"] = {r["kernel"]: {"launches": r["launches"], "us_per_launch": 1e3 * r["total_ms"] / r["launches"],
                                   "hbm_TBps": r["hbm_bytes_per_launch"] * r["launches"] / (r["total_ms"] * 1e-3) / 1e12}
                     for r in ctx.timing() if r["kernel"].startswith("kd_x_pass") and r["launches"]}
    ctx.timing_enable(False)
    print("RESULT " + json.dumps(rec), flush=True)
    dom.drop_contexts()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="128:200:1,24:1000:1,24:1000:64,256:100:1", help="npts:steps:batch,...")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--variants", default=None, help="comma-separated, in running order (default: parent if --parent-lib, full, frozen, nostack)")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--child-timeout", type=int, default=240)
    for name, typ in (("variant", str), ("fields", str), ("npts", int), ("steps", int), ("batch", int), ("round", int)):
        ap.add_argument("--" + name, type=typ, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.variant:
        return child(a)
    from spheremanopt_amd import kdyn
    variants = a.variants.split(",") if a.variants else (["parent"] if a.parent_lib else []) + ["full", "frozen", "nostack"]
    if "parent" in variants and not a.parent_lib:
        ap.error("the parent variant needs --parent-lib")
    out = open(a.out, "w") if a.out else None
    with tempfile.TemporaryDirectory() as tmp:
        made = {}
        for case in a.cases.split(","):
            N, n, B = (int(v) for v in case.split(":"))
            if N not in made:                       # the fields of a size: made once here, loaded by every child
                made[N] = os.path.join(tmp, "fields%d.npz" % N)
                np.savez(made[N], B=kdyn.synthetic_field(3 * N // 2, 1), U=kdyn.synthetic_field(3 * N // 2, 2))
            for rnd in range(a.rounds):
                for v in variants:
                    env = dict(os.environ)
                    if v == "parent":
                        env["SMO_LIB"] = os.path.abspath(a.parent_lib)
                    cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--variant", v, "--fields", made[N],
                           "--npts", str(N), "--steps", str(n), "--batch", str(B), "--round", str(rnd), "--seconds", str(a.seconds)]
                    p = subprocess.run(cmd, env=env, capture_output=True, text=True)
                    lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                    if p.returncode != 0 or not lines:
                        sys.stderr.write("%s %s round %d: exit status %d\n%s\n" % (case, v, rnd, p.returncode, p.stderr[-2000:]))
                        return 1                    # nothing more is started on the GPU after a failed point
                    print(lines[0], flush=True)
                    if out:
                        out.write(lines[0] + "\n")
                        out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
