#!/usr/bin/env python3
"""Batched KDyn (smo_config.batch): throughput of B independent gradients per call at the launch-bound sizes.

    python tools/time_kdyn_batch.py [npts ...]          default: 24 48;  SMO_TOOL_ITERS (1000), SMO_TOOL_BATCHES ("1,4,16,64,128,256")
    SMO_TOOL_RM_SPREAD="0.5,8" python tools/time_kdyn_batch.py 24      members with their own Rm against the shared one


One process, device-resident vectors.  Per (npts, B): one warm-up gradient (forward + adjoint, the HIP-graph capture at G <= 36), then
whole gradients until at least SMO_TOOL_SECONDS (1.0) have passed.  A B whose stack does not fit the HBM (SMO_ERR_NOMEM at creation) ends
that size.  With SMO_TOOL_RM_SPREAD="lo,hi" every (npts, B) is measured SMO_TOOL_ROUNDS (2) times in turn with one Rm for all members
("rm": "uniform", the geometric mean of lo and hi) and with B values spaced geometrically from lo to hi ("rm": "members", a context of
smo_create_members).  bytes_per_gradient: the kernels' compulsory HBM bytes (smo_timing_hbm_bytes x launches of one timed gradient) / B.
One JSON line per (npts, B)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from spheremanopt_amd import _capi, kdyn  # noqa: E402
from spheremanopt_amd.devvec import DeviceVector, to_device  # noqa: E402

sizes = [int(a) for a in sys.argv[1:]] or [24, 48]
n = int(os.environ.get("SMO_TOOL_ITERS", "1000"))
batches = [int(b) for b in os.environ.get("SMO_TOOL_BATCHES", "1,4,16,64,128,256").split(",")]
window = float(os.environ.get("SMO_TOOL_SECONDS", "1.0"))
Rm, dt = 1., 1e-3
spread = [float(v) for v in os.environ["SMO_TOOL_RM_SPREAD"].split(",")] if os.environ.get("SMO_TOOL_RM_SPREAD") else None
rounds = int(os.environ.get("SMO_TOOL_ROUNDS", "2")) if spread else 1
if spread:
    Rm = float(np.sqrt(spread[0] * spread[1]))


def hbm_bytes(ctx, X, g):
    """compulsory HBM bytes of one gradient of the whole batch (timing on: launch by launch, no graph)."""
    ctx.timing_enable(True)
    ctx.forward_dev(X); ctx.adjoint_dev(X, g)
    tot = sum(r["launches"] * r["hbm_bytes_per_launch"] for r in ctx.timing())
    ctx.timing_enable(False)
    return tot


for N in sizes:
    base = None
    G = 3 * N // 2
    fields = [(kdyn.synthetic_field(G, 2 * s + 1), kdyn.synthetic_field(G, 2 * s + 2)) for s in range(4)]      # cycled over the members
    fits = True
    for B, rnd, mode in [(B, r, m) for B in batches for r in range(rounds) for m in (("uniform", "members") if spread else ("uniform",))]:
        if not fits:
            break
        dom = kdyn.KDynDomain(N)
        try:
            ctx = dom.context(Rm if mode == "uniform" else np.geomspace(spread[0], spread[1], B), dt, n, "Final", batch=B)
        except _capi.SmoError as e:
            print(json.dumps({"npts": N, "batch": B, "n_iters": n, "skipped": str(e)}), flush=True)
            dom.drop_contexts()
            fits = False
            continue
        X = to_device([np.concatenate([fields[b % len(fields)][c] for b in range(B)]) for c in (0, 1)])
        g = [DeviceVector(B * ctx.vec_len), DeviceVector(B * ctx.vec_len)]
        t0 = time.perf_counter()
        ctx.forward_dev(X); ctx.adjoint_dev(X, g)
        first = time.perf_counter() - t0
        reps, t0 = 0, time.perf_counter()
        while True:
            J = ctx.forward_dev(X); ctx.adjoint_dev(X, g)
            reps += 1
            el = time.perf_counter() - t0
            if el >= window:
                break
        ms = 1e3 * el / reps
        rec = {"npts": N, "G": dom.G, "batch": B, "rm": mode, "round": rnd, "n_iters": n, "reps": reps, "window_s": el, "first_call_ms": 1e3 * first,
               "ms_per_batch": ms, "ms_per_gradient": ms / B, "gradients_per_s": 1e3 * B / ms, "graph_replays": ctx.get(2),
               "stack_bytes": ctx.stack_bytes}
        hb = hbm_bytes(ctx, X, g)
        rec["hbm_bytes_per_gradient"] = hb / B
        rec["hbm_TBps_at_measured_time"] = hb / (ms * 1e-3) / 1e12
        if base is None and B == 1:
            base = rec["gradients_per_s"]
        rec["speedup_vs_b1"] = rec["gradients_per_s"] / base if base else None
        rec["J0"] = float(J[0]) if B > 1 else float(J)
        print(json.dumps(rec), flush=True)
        del X, g
        dom.drop_contexts()
