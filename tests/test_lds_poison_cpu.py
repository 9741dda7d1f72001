"""The LDS fill suite (test_lds_poison_gpu.py) leaves no launch out and no case out, checked without a device:

- no source of the library names a launch primitive outside the one hook of csrc/smo_common.hpp (SMO_LAUNCH, SMO_LAUNCH_T, and
  SMO_LAUNCH_THE_FILL for the fill dispatch alone), so "every launch is preceded by a fill" holds by construction;
- the knob is read where a context is created and where the vector pool is entered, and nowhere else by name;
- the fill word and the rule for the knob's value of csrc/lds_poison.hpp agree with the suite's copies and with poison_ops.fill_pattern;
- the suite runs every case of poison_ops.CASES plus the one-item case, nothing hidden, nothing left out.

Limits of the source scan: it reads csrc/*.hip, *.hpp and *.cpp, not subdirectories (there are none; include/smo.h holds declarations only,
which test_include_holds_no_launch checks), and it strips `//` comments only, so a primitive named inside a block comment or a string
literal is reported as a launch (the strict side), while a launch assembled by token pasting in a macro would go unseen.
"""
import glob
import os
import re
import subprocess
import sys

import numpy as np

import poison_ops as po
import test_guard_gpu as tg
import test_lds_poison_gpu as tl

from conftest import ROOT

CSRC = os.path.join(ROOT, "spheremanopt_amd", "csrc")
PRIMITIVE = re.compile(r"hipLaunchKernelGGL|hipExtLaunchKernelGGL|hipLaunchKernel\b|hipModuleLaunchKernel|hipLaunchCooperativeKernel|<<<")


def _sources():
    files = sorted(f for ext in ("hip", "hpp", "cpp") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) >= 20 and os.path.join(CSRC, "lds_poison.hip") in files, files
    return files


def _parametrize(fn, name):
    marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize" and m.args[0] == name]
    assert len(marks) == 1, (fn.__name__, name)
    return marks[0]


def test_no_launch_outside_the_hook():
    hook_file = os.path.join(CSRC, "smo_common.hpp")
    sites = 0
    for f in _sources():
        lines = open(f).read().split("\n")
        if f == hook_file:
            begin, end = lines.index("// SMO_LAUNCH_BEGIN"), lines.index("// SMO_LAUNCH_END")
            assert begin < end
            inside = "\n".join(lines[begin:end])
            code = lines[:begin] + lines[end:]
            # the hook: three macros; the two that any file may use call lds_before_launch ahead of the primitive
            assert re.findall(r"#define (\w+)\(", inside) == ["SMO_LAUNCH", "SMO_LAUNCH_T", "SMO_LAUNCH_THE_FILL"]
            for name in ("SMO_LAUNCH", "SMO_LAUNCH_T"):
                body = inside.split("#define %s(" % name)[1].split("#define")[0]
                assert body.index("smo::lds_before_launch(stream);") < PRIMITIVE.search(body).start(), name
            assert len(PRIMITIVE.findall(inside)) == 4                # SMO_LAUNCH 1, SMO_LAUNCH_T 2 (stamped or not), the fill 1
        else:
            code = lines
        code = [l.split("//")[0] for l in code]                       # (comments may speak of the primitives)
        for l in code:
            assert not PRIMITIVE.search(l), "%s: a raw launch outside the hook: %s" % (os.path.basename(f), l.strip())
        text = "\n".join(code)
        sites += len(re.findall(r"\bSMO_LAUNCH(?:_T)?\(", text)) if f != hook_file else 0
        # the unfilled launch is the fill dispatch's own and nobody else's
        n_fill = len(re.findall(r"\bSMO_LAUNCH_THE_FILL\(", text))
        assert n_fill == (1 if os.path.basename(f) == "lds_poison.hip" else 0), (f, n_fill)
    assert sites >= 76, sites                                        # 75 launch expressions in 8 files when the hook came, and the probe's


def test_include_holds_no_launch():
    for f in glob.glob(os.path.join(ROOT, "include", "*")):
        assert not PRIMITIVE.search(open(f).read()) and "SMO_LAUNCH" not in open(f).read(), f
    assert not [d for d in os.listdir(CSRC) if os.path.isdir(os.path.join(CSRC, d)) and d != "build"]


def test_the_fill_dispatch_is_the_fill_kernel_and_waits_for_nobody():
    src = open(os.path.join(CSRC, "lds_poison.hip")).read()
    assert re.search(r"SMO_LAUNCH_THE_FILL\(lds_fill_kernel,", src)
    kernel = src.split("void lds_fill_kernel(")[1].split("\n}\n")[0]
    assert not re.search(r"atomic|while|__threadfence|hipcooperative|grid\.sync", kernel, re.I), kernel
    assert len(re.findall(r"s_sleep", kernel)) <= 4


def test_the_knob_is_read_at_context_creation_and_at_the_vector_pool():
    named, readers = [], {}
    for f in _sources():
        text = open(f).read()
        code = "\n".join(l.split("//")[0] for l in text.split("\n"))
        if '"SMO_POISON_LDS"' in code:
            named.append(os.path.basename(f))
        readers[os.path.basename(f)] = len(re.findall(r"\blds_poison_read\(\)", code))
    assert named == ["lds_poison.hip"]                               # one getenv, in the one reader
    assert readers["common.cpp"] == 1 and readers["vecops.hip"] == 1
    base_init = open(os.path.join(CSRC, "common.cpp")).read().split("int Context::base_init() {")[1].split("\n}\n")[0]
    pool_for = open(os.path.join(CSRC, "vecops.hip")).read().split("int pool_for(")[1].split("\n}\n")[0]
    assert "SMO_TRY(lds_poison_read());" in base_init and "SMO_TRY(lds_poison_read());" in pool_for
    hook = open(os.path.join(CSRC, "smo_common.hpp")).read().split("inline void lds_before_launch(")[1].split("\n}\n")[0]
    assert "getenv" not in hook and hook.count("g_lds_poison.load(") == 1


def test_the_suite_mirrors_the_header(tmp_path):
    """fill_word and the rule for the knob's value against lds_poison.hpp, through a small program (g++ alone compiles the header)."""
    bytes_ = [0, 1, 63, 127, 128, 255]
    values = list(tl.BAD_VALUES) + ["0", "7", "63", "255", "007", "banded", "25 5", "+5"]
    src = tmp_path / "mirror.cpp"
    src.write_text('#include <cstdio>\n#include "lds_poison.hpp"\nint main() {\nint b = 0;\n' +
                   "".join('std::printf("%%llu\\n", (unsigned long long)smo::lds::fill_word(%d));\n' % b for b in bytes_) +
                   "".join('std::printf("%%d\\n", smo::lds::parse_byte("%s", &b) ? b : -1);\n' % v for v in values) + "return 0; }\n")
    exe = str(tmp_path / "mirror")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:len(bytes_)] == [tl.fill_word(b) for b in bytes_]
    assert got[len(bytes_):] == [-1] * len(tl.BAD_VALUES) + [0, 7, 63, 255, 7, -1, -1, -1]
    for b in bytes_:                                                 # ... and the word is eight copies of the byte, as SMO_POISON's fill
        assert po.same_bits(np.array([tl.fill_word(b)], dtype=np.uint64).view(np.float64), po.fill_pattern(b, 1))
    assert np.isnan(po.fill_pattern(255, 1)[0]) and 4.7e-4 < po.fill_pattern(63, 1)[0] < 4.9e-4


def test_the_lds_suite_runs_every_case_of_the_poison_table():
    want = [c["id"] for c in po.CASES]
    m = _parametrize(tl.test_no_path_reads_lds_it_did_not_write, "case")
    cases, ids = list(m.args[1]), list(m.kwargs["ids"])
    assert ids[:len(want)] == want and len(cases) == len(want) + 1
    assert all(a is b for a, b in zip(cases, po.CASES))               # the table itself, in its order: no copy that could drift
    assert cases[-1] is tg.ONE_ITEM and ids[-1] == "kdyn-128-one_item_per_thread-Final-Discrete" and len(set(ids)) == len(ids)
    assert all(type(c) is dict for c in cases)                       # no pytest.param that could carry a mark
    assert {mk.name for mk in tl.test_no_path_reads_lds_it_did_not_write.pytestmark} == {"parametrize"}
    assert getattr(tl.pytestmark, "name", None) == "gpu"
    src = open(os.path.join(ROOT, "tests", "test_lds_poison_gpu.py")).read()
    assert not re.search(r"\b(skip|skipif|xfail|importorskip)\b", src)


def test_the_other_case_lists_of_the_lds_suite():
    assert tl.FILLS == (255, 63)
    assert tl.PROBE_BYTES == (1024, 40960, 65536, 163840) and tl.PROBE_GRIDS == (1, 4)
    assert tl.BAD_VALUES == ("256", "-1", "1.0", "", " 7", "0x3F")
    assert list(_parametrize(tl.test_device_vector_algebra_under_the_lds_fill, "n").args[1]) == list(tg.VEC_SIZES)
    assert [c["id"] for c in _parametrize(tl.test_lds_fill_poison_and_guard_together, "case").args[1]] == list(tg.BOTH_KNOBS)
    assert list(_parametrize(tl.test_the_knob_moves_no_byte_count_and_no_path, "family").args[1]) == sorted(tg.SMALL)


def test_the_lds_suite_imports_without_loading_the_library():
    code = ("import sys, test_lds_poison_gpu; from spheremanopt_amd import _capi; assert _capi._lib is None; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('oracle', 'torch')]; assert not bad, bad; print(len(test_lds_poison_gpu.CASES))")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")])))
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == len(po.CASES) + 1
