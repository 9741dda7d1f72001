#!/usr/bin/env python3
"""What an exact SH23 Hessian-vector product costs against the two forward+adjoint pairs a central difference of gradients needs.

On one context per configuration, device-resident vectors: milliseconds per hessvec (tangent sweep + second-order adjoint sweep) and per
forward+adjoint pair, at Npts = 256, N = 500, batch 1 and batch 256, through the instantiated kernels and (SMO_SH_ANY=1) the any-length
ones.  Warm-up first; every figure is the median of the repeats, each repeat one synchronous call timed on the host; the split into the
two sweeps comes from the context's timing classes (HIP events on its stream) in a second pass, so that the events stay out of the
wall-clock figures.  A child process per configuration: the knob is read when the context is created and the runs do not share a process.

With --parent-lib (libsmo.so of ANOTHER build, e.g. the parent commit's) every configuration runs on both builds, parent and this tree
taking turns for --rounds rounds, a child process each (a process binds one library, through SMO_LIB); every round is written out, and
per configuration and figure a summary line compares the medians over the rounds: this tree's may exceed the parent's by no more than the
parent's own range over its rounds (max - min), the noise the machine shows on unchanged code.  A child that ends abnormally ends the run.

usage: python tools/time_sh23_hessvec.py [--out profiles/r13_sh23_hessvec.jsonl] [--repeats 15] [--npts 256] [--n-iters 500]
                                         [--parent-lib /path/to/parent/libsmo.so] [--rounds 3]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def measure(npts, n_iters, batch, repeats):
    import numpy as np

    from spheremanopt_amd import _capi, sh23
    from spheremanopt_amd.devvec import DeviceVector
    dom = sh23.SH23Domain(npts)
    G = dom.G
    X = np.concatenate([sh23._band_limited_noise(dom, 42 + b, 0.0725) for b in range(batch)])
    V = np.concatenate([sh23._band_limited_noise(dom, 1007 + b, 0.0725) for b in range(batch)])
    ctx = _capi.Context(_capi.SMO_SH23, npts, dom.interval, 0.1, n_iters, sh23.A_PARAM, batch=batch)
    dX, dV, dG, dH = DeviceVector.from_numpy(X), DeviceVector.from_numpy(V), DeviceVector(batch * G), DeviceVector(batch * G)

    def pair():
        ctx.forward_dev([dX])
        ctx.adjoint_dev([dX], [dG])

    def product():
        ctx.hessvec_dev([dV], [dH])

    def median_ms(fn):
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts))

    for _ in range(3):                                       # warm-up: code objects, the tangent stack, clocks
        pair()
        product()
    rec = {"npts": npts, "n_iters": n_iters, "batch": batch, "any": os.environ.get("SMO_SH_ANY", "0") == "1", "repeats": repeats,
           "pair_ms": median_ms(pair), "hessvec_ms": median_ms(product)}
    rec["hessvec_over_pair"] = rec["hessvec_ms"] / rec["pair_ms"]
    ctx.timing_enable(True)
    for _ in range(repeats):
        pair()
        product()
    for t in ctx.timing():
        if t["launches"]:
            rec[t["kernel"] + "_ms"] = t["total_ms"] / t["launches"]
    ctx.timing_enable(False)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_sh23_hessvec.jsonl"))
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--npts", type=int, default=256)
    ap.add_argument("--n-iters", type=int, default=500)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=None, help="per build (default: 3 with --parent-lib, else 1)")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--one", nargs=2, metavar=("BATCH", "ANY"), help="(internal) measure one configuration and print its record")
    a = ap.parse_args()
    if a.one:
        print("REC " + json.dumps(measure(a.npts, a.n_iters, int(a.one[0]), a.repeats)), flush=True)
        return 0
    builds = (["parent"] if a.parent_lib else []) + ["commit"]
    rounds = a.rounds or (3 if a.parent_lib else 1)
    out = open(a.out, "w")
    for any_len in ("0", "1"):
        for batch in (1, 256):
            recs = {b: [] for b in builds}
            for rnd in range(rounds):
                for build in builds:
                    env = dict(os.environ, SMO_SH_ANY=any_len)
                    env.pop("SMO_LIB", None)
                    if build == "parent":
                        env["SMO_LIB"] = os.path.abspath(a.parent_lib)
                    p = subprocess.run(["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--one", str(batch), any_len,
                                        "--repeats", str(a.repeats), "--npts", str(a.npts), "--n-iters", str(a.n_iters)], env=env, capture_output=True, text=True)
                    lines = [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("REC ")]
                    if p.returncode != 0 or not lines:
                        sys.stderr.write("configuration batch=%d SMO_SH_ANY=%s, %s build, round %d: exit status %d\n%s\n" % (batch, any_len, build, rnd, p.returncode, p.stderr[-2000:]))
                        return 1                             # nothing more is started on the GPU after a failed point
                    rec = json.loads(lines[0])
                    if a.parent_lib:
                        rec = dict(build=build, round=rnd, **rec)
                    recs[build].append(rec)
                    print(json.dumps(rec), flush=True)
                    out.write(json.dumps(rec) + "\n")
                    out.flush()
            if a.parent_lib:
                summary = {"summary": True, "batch": batch, "any": any_len == "1", "rounds": rounds, "figures": {}}
                for key in [k for k in recs["commit"][0] if k.endswith("_ms")]:
                    par, com = sorted(r[key] for r in recs["parent"]), sorted(r[key] for r in recs["commit"])
                    med = lambda v: v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
                    summary["figures"][key] = {"parent_median": med(par), "commit_median": med(com), "parent_range": par[-1] - par[0],
                                               "within": med(com) - med(par) <= par[-1] - par[0]}
                print(json.dumps(summary), flush=True)
                out.write(json.dumps(summary) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
