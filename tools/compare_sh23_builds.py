#!/usr/bin/env python3
"""Do two builds of the library compute the same SH23 bits?  Seeded cases on this tree's libsmo.so and on ANOTHER build (--parent-lib:
libsmo.so of the parent commit), compared byte for byte: J, the Discrete and the Continuous gradient, dJ, H.V and the snapshots
0, 1, N/2, N of every member.

    python tools/compare_sh23_builds.py --parent-lib /path/to/parent/libsmo.so [--lib /path/to/another/libsmo.so]
                                        [--out profiles/r16_sh23_sweeps_bits_parent_vs_commit.jsonl]

Cases, N = 6 steps each: the instantiated lengths 16, 150, 256, 512, 600, 768, 800, 1024 (one and several rounds of the per-mode loop, both
forms of the second-order sweep); the any-length 21, 54, 97, 1100 (odd, LDS opt-in); 64 under SMO_SH_ANY=1; a batch of 3 with one `a` per
member and the horizons (N, N-1, 1) at 64 and at 54.  One child process per library (a process binds one library, through SMO_LIB), each
under its own time limit; a child that ends abnormally ends the run.  One JSON line per case with the SHA-256 of every result on both
builds and, for a result that differs, how many of its entries do and by how much at most; exit status 1 if any differs."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

N = 6
CASES = ([{"npts": n} for n in (16, 150, 256, 512, 600, 768, 800, 1024, 21, 54, 97, 1100)] + [{"npts": 64, "any": True}]
         + [{"npts": n, "a": (-0.3, -0.2, -0.25), "horizons": (N, N - 1, 1)} for n in (64, 54)])


def name(case):
    return "npts%d%s%s" % (case["npts"], "_any" if case.get("any") else "", "_batch3_members_horizons" if "a" in case else "")


def run_case(case, keep):
    import numpy as np

    from spheremanopt_amd import _capi, sh23
    os.environ["SMO_SH_ANY"] = "1" if case.get("any") else "0"          # read when the context is created
    npts, a, hz = case["npts"], case.get("a", sh23.A_PARAM), case.get("horizons")
    batch = len(a) if hz else 1
    dom = sh23.SH23Domain(npts)
    X = np.concatenate([sh23._band_limited_noise(dom, 42 + b, 0.0725) for b in range(batch)])
    V = np.concatenate([sh23._band_limited_noise(dom, 1007 + b, 0.0725) for b in range(batch)])
    ctx = _capi.Context(_capi.SMO_SH23, npts, dom.interval, 0.02 if npts > 256 else 0.1, N, a, batch=batch)
    if hz:
        ctx.set_horizons(hz)
    res = {"J": np.atleast_1d(ctx.forward([X])), "grad_discrete": ctx.adjoint(adjoint_type="Discrete")[0],
           "grad_continuous": ctx.adjoint(adjoint_type="Continuous")[0]}
    (HV,), dJ = ctx.hessvec([V])
    res["dJ"], res["HV"] = np.atleast_1d(dJ), HV
    for b in range(batch):
        n = hz[b] if hz else N
        for i in (0, 1, n // 2, n):
            res["snapshot_b%d_%d" % (b, i)] = np.array(ctx.snapshot(i, b))
    ctx.close()
    bad = [k for k, v in res.items() if not np.all(np.isfinite(v))]
    if bad:
        raise SystemExit("%s: not finite: %s" % (name(case), bad))
    np.savez(os.path.join(keep, name(case) + ".npz"), **res)
    return {k: hashlib.sha256(np.ascontiguousarray(v, dtype=np.float64).tobytes()).hexdigest() for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--lib", default=None, help="the build compared with it (default: this tree's; the parent's again: is a build equal to itself?)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)       # the directory this child leaves its arrays in
    a = ap.parse_args()
    if a.child:
        for case in CASES:
            print("DIGESTS " + json.dumps({"case": name(case), "sha256": run_case(case, a.child)}), flush=True)
        return 0
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    import numpy as np
    got, tmp = {}, tempfile.TemporaryDirectory()
    for build, lib in (("parent", os.path.abspath(a.parent_lib)), ("commit", os.path.abspath(a.lib) if a.lib else None)):
        os.mkdir(os.path.join(tmp.name, build))
        env = dict(os.environ)
        env.pop("SMO_LIB", None)
        if lib:
            env["SMO_LIB"] = lib
        p = subprocess.run(["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child",
                            os.path.join(tmp.name, build)], env=env,
                           capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write("%s build: exit status %d\n%s\n%s\n" % (build, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
            return 2                                         # nothing more is started on the GPU after a failed child
        got[build] = {r["case"]: r["sha256"] for r in (json.loads(ln[8:]) for ln in p.stdout.splitlines() if ln.startswith("DIGESTS "))}
    out = open(a.out, "w") if a.out else None
    differ = 0
    for case in CASES:
        par, com = got["parent"][name(case)], got["commit"][name(case)]
        diff = {}
        if par != com:
            pa, ca = (np.load(os.path.join(tmp.name, b, name(case) + ".npz")) for b in ("parent", "commit"))
            for k in sorted(k for k in par if par[k] != com.get(k)):
                x, y = pa[k].reshape(-1), ca[k].reshape(-1)
                ne = x.view(np.uint64) != y.view(np.uint64)
                diff[k] = {"entries": int(ne.sum()), "of": int(x.size), "max_abs_diff": float(np.abs(x - y).max()), "max_abs": float(np.abs(x).max()),
                           "first": [int(np.flatnonzero(ne)[0]), float(x[ne][0]), float(y[ne][0])]}
        differ += bool(diff)
        line = json.dumps({"case": name(case), "n_iters": N, "equal": not diff, "differ": diff, "parent": par, "commit": com})
        print("%-40s %s" % (name(case), "equal (%d results)" % len(par) if not diff else "DIFFER: " + json.dumps(diff)), flush=True)
        if out:
            out.write(line + "\n")
    print("%d of %d cases differ" % (differ, len(CASES)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
