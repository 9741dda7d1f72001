"""Guard zones of SMO_GUARD on the CPU (spheremanopt_amd/csrc/guard.hpp): tests/c/guard_host_test.cpp checks the knob's values, the zone-size
rule at its three regimes and their boundaries, the pattern (no word is zero or a poison fill, none repeats) and the comparison (one damaged
byte at the first, the last and an interior position of each zone is reported at that offset; damage in slack of every length 0 .. 255; an
intact block reports nothing).  A program of its own: nothing is loaded into Python."""
import os
import subprocess

from conftest import ROOT

GROUPS = ("knob", "zone rule", "pattern", "intact", "single byte", "slack")


def _compile(out, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "spheremanopt_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "guard_host_test.cpp"), "-o", out], capture_output=True, text=True)


def test_zone_rule_pattern_and_comparison(tmp_path):
    """Built with the address and undefined-behaviour sanitizers where the host compiler has them."""
    out = str(tmp_path / "guard_host_test")
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


def test_the_knob_is_read_in_one_place():
    """Both allocation sites call the one helper: no other source names the variable."""
    csrc = os.path.join(ROOT, "spheremanopt_amd", "csrc")
    readers = [f for f in sorted(os.listdir(csrc)) if os.path.isfile(os.path.join(csrc, f)) and 'getenv("SMO_GUARD")' in open(os.path.join(csrc, f)).read()]
    assert readers == ["guard.hip"]
    for f, site in (("common.cpp", "DevPool::alloc"), ("vecops.hip", "smo_vec_alloc")):
        src = open(os.path.join(csrc, f)).read()
        assert "guard_cap(" in src and "guard_malloc(" in src and "guard_check(" in src, site
        assert "hipMalloc(" not in src.replace("hipMalloc(%zu", ""), site          # (the message text aside) no allocation round the helper
