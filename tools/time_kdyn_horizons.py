#!/usr/bin/env python3
"""KDyn members with a horizon of their own (smo_set_horizons): what existing contexts pay for the feature, and what a sweep over H horizons
costs in one call.  Milliseconds per gradient (forward + adjoint, device-resident vectors), "Final" cost.

  1. existing contexts (--existing npts:steps:batch,...): a plain context that never sets a horizon, on
         parent   ANOTHER build of the library (--parent-lib: libsmo.so of the parent commit)
         this     this tree
     taking turns inside every round (measuring guide: interleave, repeat, report every round).
  2. the sweep (--sweeps npts:capacity:H,...): horizons capacity * (b + 1) / H, b = 0 .. H-1, full and frozen-velocity contexts, as
         sweep     ONE context of H members with those horizons: one forward + one adjoint call per sweep
         sequence  H batch-1 contexts of n_iters = N_b, called one after another
         uniform   ONE plain batch of H members at the capacity (every member runs all the steps)
     ms per sweep, and  ideal = sum(N_b) / (H * capacity) * uniform: the time of the sweep if idle members gave all of theirs back.

    python tools/time_kdyn_horizons.py --parent-lib /path/to/parent/libsmo.so [--out profiles/r11_kdyn_horizons.jsonl]
                                       [--existing 24:1000:1,24:1000:64,128:200:1] [--sweeps 24:1000:16,128:200:4] [--rounds 2] [--seconds 1.0]

Every point runs in a process of its own (a process binds one library) under its own time limit; a child that ends abnormally ends the
run.  Per point: one warm-up gradient (graph capture at G <= 36), then whole gradients until `--seconds` have passed.  One JSON line per
point; without --parent-lib the parent variant is left out."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def horizons(cap, H):
    return tuple(cap * (b + 1) // H for b in range(H))


def child(a):
    from spheremanopt_amd import _capi
    if a.variant == "parent":                       # an older library may lack the newest entry points: bind what it has
        import ctypes
        L = ctypes.CDLL(_capi.LIB_PATH)
        for name in [n for n in _capi.SIGNATURES if not hasattr(L, n)]:
            _capi.SIGNATURES.pop(name)
    from spheremanopt_amd import kdyn
    from spheremanopt_amd.devvec import DeviceVector, to_device
    N, n, B = a.npts, a.steps, a.batch
    f = np.load(a.fields)
    dom = kdyn.KDynDomain(N)
    kw = {"frozen_U": True} if a.frozen else {}
    ng = 1 if a.frozen else 2
    hz = horizons(n, B)
    if a.variant == "sequence":
        runs = [(dom.context(1.0, 1e-3, nb, "Final", **kw), 1) for nb in hz]
    elif a.variant == "sweep":
        runs = [(dom.context(1.0, 1e-3, hz, "Final", **kw), B)]
    else:                                           # parent, this, uniform: a plain context
        runs = [(dom.context(1.0, 1e-3, n, "Final", batch=B, **kw), B)]
    vec = {m: (to_device([np.tile(f["B"], m), np.tile(f["U"], m)]), [DeviceVector(m * dom.vec_len) for _ in range(ng)]) for m in {m for _, m in runs}}

    def gradient():
        for ctx, m in runs:
            X, g = vec[m]
            J = ctx.forward_dev(X)
            ctx.adjoint_dev(X, g)
        return J

    t0 = time.perf_counter()
    gradient()
    first = time.perf_counter() - t0
    reps, t0 = 0, time.perf_counter()
    while True:
        J = gradient()
        reps += 1
        el = time.perf_counter() - t0
        if el >= a.seconds:
            break
    rec = {"variant": a.variant, "frozen": bool(a.frozen), "round": a.round, "npts": N, "G": dom.G, "n_iters": n, "batch": B, "reps": reps,
           "window_s": el, "first_call_ms": 1e3 * first, "ms_per_sweep": 1e3 * el / reps, "graph_replays": sum(c.get(2) for c, _ in runs),
           "J_last": float(np.atleast_1d(J)[-1]), "lib": "--parent-lib build" if a.variant == "parent" else "this tree"}
    if a.variant in ("sweep", "sequence"):
        rec["horizons"] = list(hz)
    print("RESULT " + json.dumps(rec), flush=True)
    dom.drop_contexts()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--existing", default="24:1000:1,24:1000:64,128:200:1", help="npts:steps:batch,... ('' = none)")
    ap.add_argument("--sweeps", default="24:1000:16,128:200:4", help="npts:capacity:H,... ('' = none)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--frozen", type=int, default=0, help=argparse.SUPPRESS)
    for name, typ in (("variant", str), ("fields", str), ("npts", int), ("steps", int), ("batch", int), ("round", int)):
        ap.add_argument("--" + name, type=typ, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.variant:
        return child(a)
    from spheremanopt_amd import kdyn
    points = []                                     # (npts, steps, batch, round, variant, frozen), in running order
    for case in filter(None, a.existing.split(",")):
        N, n, B = (int(v) for v in case.split(":"))
        for rnd in range(a.rounds):
            points += [(N, n, B, rnd, v, 0) for v in ((["parent"] if a.parent_lib else []) + ["this"])]
    for case in filter(None, a.sweeps.split(",")):
        N, n, H = (int(v) for v in case.split(":"))
        for rnd in range(a.rounds):
            points += [(N, n, H, rnd, v, fr) for fr in (0, 1) for v in ("sweep", "sequence", "uniform")]
    out = open(a.out, "w") if a.out else None
    with tempfile.TemporaryDirectory() as tmp:
        made = {}
        for N, n, B, rnd, v, fr in points:
            if N not in made:                       # the fields of a size: made once here, loaded by every child
                made[N] = os.path.join(tmp, "fields%d.npz" % N)
                np.savez(made[N], B=kdyn.synthetic_field(3 * N // 2, 1), U=kdyn.synthetic_field(3 * N // 2, 2))
            env = dict(os.environ)
            if v == "parent":
                env["SMO_LIB"] = os.path.abspath(a.parent_lib)
            cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--variant", v, "--fields", made[N],
                   "--npts", str(N), "--steps", str(n), "--batch", str(B), "--round", str(rnd), "--seconds", str(a.seconds), "--frozen", str(fr)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True)
            lines = [ln[7:] for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                sys.stderr.write("%d:%d:%d %s round %d: exit status %d\n%s\n" % (N, n, B, v, rnd, p.returncode, p.stderr[-2000:]))
                return 1                            # nothing more is started on the GPU after a failed point
            print(lines[0], flush=True)
            if out:
                out.write(lines[0] + "\n")
                out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
