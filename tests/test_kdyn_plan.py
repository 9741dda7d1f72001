"""Checkpoint schedule of the KDYN and Poiseuille contexts (spheremanopt_amd/csrc/ckpt_plan.hpp) and HBM plan of the KDYN context
(kdyn_plan.hpp) on the CPU: tests/c/kdyn_plan_test.cpp walks the slot map, the forward solve, both adjoint sweeps and out-of-order snapshot
reads of every schedule with N <= 40, Poiseuille's (state N always kept, never written by a replay) among them, compares Poiseuille's slot
map with the formulas pois.hip held before, and compares the choices made from the free HBM (both interval searches, dense tail, Ty stack,
Ty cache) and the list of tuned sizes with brute-force answers.  A program of its own: nothing is loaded into Python."""
import os
import subprocess

from conftest import ROOT

GROUPS = ("slot map", "sweeps", "old poiseuille slot map", "poiseuille interval", "dense tail", "forced tail", "interval", "ty buffers", "flagship", "tuned list")


def _compile(out, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "spheremanopt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "kdyn_plan_test.cpp"), "-o", out], capture_output=True, text=True)


def test_schedule_and_hbm_plan(tmp_path):
    """Built with the address and undefined-behaviour sanitizers where the host compiler has them."""
    out = str(tmp_path / "kdyn_plan_test")
    r = _compile(out, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0:                                                  # a compiler without the sanitizer runtimes
        print("sanitizers unavailable:", r.stderr[-300:])
        r = _compile(out, [])
    assert r.returncode == 0, r.stderr
    r = subprocess.run([out], capture_output=True, text=True)
    print(r.stdout[-1500:])
    ok = [ln for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(ok) == len(GROUPS) and all(ln.startswith("ok " + g + " (") for ln, g in zip(ok, GROUPS)), r.stdout
    assert "ok dense tail (16220 cases)" in r.stdout
