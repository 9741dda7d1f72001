#!/usr/bin/env python3
"""Batched plane-Poiseuille (smo_config.batch, Discrete formulation): throughput of B independent gradients per call that share one set of
tau operators, and the operator bytes a member costs.

    python tools/time_pois_batch.py [--ckpt k] [NxxNz ...]    default: 48x36 96x48 384x192; --ckpt: the checkpoint interval of every
                                                        context (smo_config.ckpt; 1 = keep every snapshot, the default)
    SMO_TOOL_ITERS (1000)  SMO_TOOL_S (1: mix-norm)  SMO_TOOL_SECONDS (1.0)
    SMO_TOOL_BATCHES ("1,2,4,8,16,32,64,128,256")       a B whose stack does not fit the HBM (SMO_ERR_NOMEM at creation) ends that size
    SMO_TOOL_MBS ("0")                                  members per workgroup of the HODLR apply for B > 1, comma-separated: 0 = the library's
                                                        choice, 1 | 2 | 4 = forced through SMO_POIS_APPLY_MB
    SMO_TOOL_MAX_GB (200)                               skip a B whose snapshot stack would be larger

One process, device-resident vectors.  Per (size, B, MB): one warm-up gradient (forward + adjoint), then whole gradients until at least
SMO_TOOL_SECONDS have passed.  hbm_bytes_per_gradient_per_member: the kernels' compulsory HBM bytes (smo_timing_hbm_bytes x launches of one
timed gradient) / B — the operator stream of the two applies, read once per group of MB members.  speedup_vs_b1: gradients/s over those of
B = 1 in the same run.  One JSON line per (size, B, MB)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from spheremanopt_amd import _capi, poiseuille as pz  # noqa: E402
from spheremanopt_amd.devvec import DeviceVector, to_device  # noqa: E402

argv, ckpt = sys.argv[1:], 1
if "--ckpt" in argv:
    i = argv.index("--ckpt")
    ckpt = int(argv[i + 1])
    del argv[i:i + 2]
sizes = [tuple(int(v) for v in a.split("x")) for a in argv] or [(48, 36), (96, 48), (384, 192)]
n = int(os.environ.get("SMO_TOOL_ITERS", "1000"))
s = int(os.environ.get("SMO_TOOL_S", "1"))
batches = [int(b) for b in os.environ.get("SMO_TOOL_BATCHES", "1,2,4,8,16,32,64,128,256").split(",")]
mbs = [int(m) for m in os.environ.get("SMO_TOOL_MBS", "0").split(",")]
window = float(os.environ.get("SMO_TOOL_SECONDS", "1.0"))
max_gb = float(os.environ.get("SMO_TOOL_MAX_GB", "200"))
Re, Ri, dt, Pr, delta = 500., 0.05, 5e-3, 1., 0.125


def hbm_bytes(ctx, X, g):
    """compulsory HBM bytes of one gradient of the whole batch, and the kernel time of the apply classes"""
    ctx.timing_enable(True)
    ctx.forward_dev(X); ctx.adjoint_dev(X, g)
    t = ctx.timing()
    ctx.timing_enable(False)
    tot = sum(r["launches"] * r["hbm_bytes_per_launch"] for r in t)
    apply_us = {r["kernel"]: 1e3 * r["total_ms"] / r["launches"] for r in t if r["kernel"].startswith("pois_apply") and r["launches"]}
    return tot, apply_us


for Nx, Nz in sizes:
    base, stop = None, False
    amps = (1., 3., 0.3, 2.)                                            # cycled over the members
    fields = [a * 1e-3 * np.random.RandomState(5 + i).standard_normal(2 * Nx * Nz) for i, a in enumerate(amps)]
    for B in batches:
        if stop:
            break
        for mb in (mbs if B > 1 else [0]):
            if mb:
                os.environ["SMO_POIS_APPLY_MB"] = str(mb)
            else:
                os.environ.pop("SMO_POIS_APPLY_MB", None)
            rec = {"Nx": Nx, "Nz": Nz, "batch": B, "apply_mb": mb or "default", "n_iters": n, "s": s, "ckpt": ckpt}
            slots = n + 1 if ckpt == 1 else (n // ckpt + ckpt + 1 if ckpt > 1 else 0)          # (an upper bound; ckpt = 0 sizes itself)
            stack_gb = B * slots * 3 * 2 * ((Nx - 1) // 2 + 1) * Nz * 8 / 1e9
            if stack_gb > max_gb:
                print(json.dumps(dict(rec, skipped="snapshot stack of %.0f GB" % stack_gb)), flush=True)
                stop = True
                break
            dom = pz.PoiseuilleDomain(Nx, Nz, ckpt=ckpt)
            t0 = time.perf_counter()
            try:
                ctx = dom.context(Re, Ri, n, dt, s, Pr, delta, batch=B)
            except _capi.SmoError as e:
                print(json.dumps(dict(rec, skipped=str(e))), flush=True)
                dom.drop_contexts()
                stop = True
                break
            rec["create_s"] = time.perf_counter() - t0
            X = to_device([np.concatenate([fields[b % len(fields)] for b in range(B)])])
            g = [DeviceVector(B * ctx.vec_len)]
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
            rec.update({"reps": reps, "window_s": el, "first_call_ms": 1e3 * first, "ms_per_batch": ms, "ms_per_gradient": ms / B,
                        "gradients_per_s": 1e3 * B / ms, "stack_bytes": ctx.stack_bytes, "ckpt_in_use": int(ctx.get(0))})
            hb, apply_us = hbm_bytes(ctx, X, g)
            rec["hbm_bytes_per_gradient_per_member"] = hb / B
            rec["apply_us_per_launch"] = apply_us
            if base is None and B == 1:
                base = rec["gradients_per_s"]
            rec["speedup_vs_b1"] = rec["gradients_per_s"] / base if base else None
            rec["J0"] = float(J[0]) if B > 1 else float(J)
            print(json.dumps(rec), flush=True)
            del X, g
            dom.drop_contexts()
