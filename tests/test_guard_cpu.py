"""The guard suite (test_guard_gpu.py) runs every case of poison_ops.CASES — nothing hidden, nothing skipped — plus the one-item shape of the
adjoint x pass of test_kdyn_adj_x_shape_gpu.py, and its own copies of the zone rule and of the pattern agree with csrc/guard.hpp.  No device
call here: the modules import without the library being loaded."""
import os
import re
import subprocess
import sys

import poison_ops as po
import test_guard_gpu as tg

from conftest import ROOT


def _parametrize(fn, name):
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize" and m.args[0] == name]
    assert len(marks) == 1, (fn.__name__, name)
    return marks[0]


def test_the_guard_suite_runs_every_case_of_the_poison_table():
    want = [c["id"] for c in po.CASES]
    m = _parametrize(tg.test_no_path_writes_outside_its_blocks, "case")
    cases, ids = list(m.args[1]), list(m.kwargs["ids"])
    assert ids[:len(want)] == want and cases[:len(want)] == po.CASES                 # the table itself, in its order: no copy that could drift
    assert all(a is b for a, b in zip(cases, po.CASES))
    assert ids[len(want):] == ["kdyn-128-one_item_per_thread-Final-Discrete"] and len(set(ids)) == len(ids)
    extra = cases[-1]
    assert extra["family"] == "kdyn" and extra["size"] == 128 and extra["n"] == 3 and extra["env"] == {"SMO_KD_ADJ_SEQ_ITEMS": "1"}
    # every id is run: plain dictionaries (no pytest.param that could carry a skip or xfail mark), and no such mark on the test or the module
    assert all(type(c) is dict for c in cases)
    names = {mk.name for mk in tg.test_no_path_writes_outside_its_blocks.pytestmark}
    assert names == {"parametrize"}
    assert getattr(tg.pytestmark, "name", None) == "gpu"
    src = open(os.path.join(ROOT, "tests", "test_guard_gpu.py")).read()
    assert not re.search(r"\b(skip|skipif|xfail|importorskip)\b", src)


def test_the_other_case_lists_of_the_guard_suite():
    by = {c["id"]: c for c in po.CASES}
    assert all(i in by for i in tg.BOTH_KNOBS) and sorted(by[i]["family"] for i in tg.BOTH_KNOBS) == ["kdyn", "pois", "sh23", "shb23"]
    assert [c["id"] for c in _parametrize(tg.test_guard_and_poison_together, "case").args[1]] == list(tg.BOTH_KNOBS)
    assert sorted(tg.SMALL) == ["kdyn", "pois", "sh23", "shb23"]
    assert set(po.VEC_SIZES) | {31, 32, 33, 2 * 4096 * 256 + 1537} == set(tg.VEC_SIZES)
    assert [(8 * n + 255) // 256 * 256 - 8 * n for n in (31, 32, 33)] == [8, 0, 248]           # slack, bytes
    assert tg.CAP == 64 << 20
    assert tg.BAD_VALUES == ("100", "0", "-4096", "4096.0", "", " 4096", "2147483648")


def test_the_suite_mirrors_the_header(tmp_path):
    """zone_bytes and guard_word of test_guard_gpu.py against guard.hpp, through a small program (g++ alone compiles the header)."""
    reqs = [1, 255, 256, 257, 264, 4096, 4097, tg.CAP - 1, tg.CAP, tg.CAP + 1, 10 * tg.CAP]
    words = [(1, 0), (1, 511), (2, 0), (2, 31), (2, 542), (2, (1 << 27) + 5)]
    src = tmp_path / "mirror.cpp"
    src.write_text('#include <cstdio>\n#include "guard.hpp"\nint main() {\n' +
                   "".join('std::printf("%%zu\\n", smo::guard::zone_bytes(%dull, %dull));\n' % (r, tg.CAP) for r in reqs) +
                   "".join('std::printf("%%llu\\n", (unsigned long long)smo::guard::word(%d, %dull));\n' % w for w in words) + "return 0; }\n")
    exe = str(tmp_path / "mirror")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "spheremanopt_amd", "csrc"), str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [tg.zone_bytes(r) for r in reqs] + [tg.guard_word(*w) for w in words]


def test_the_guard_suite_imports_without_loading_the_library():
    code = ("import sys, test_guard_gpu; from spheremanopt_amd import _capi; assert _capi._lib is None; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('oracle', 'torch')]; assert not bad, bad; print(len(test_guard_gpu.CASES))")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")])))
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == len(po.CASES) + 1
