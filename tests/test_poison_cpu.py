"""The case table of poison_ops.py names every path, knob value and size test_poison_gpu.py has to run, each exactly once; and poison_ops
imports without the library (numpy only), like the other *_ops modules."""
import subprocess
import sys

import poison_ops as po

TWO = sorted([("Integrated", "Continuous"), ("Final", "Discrete")], key=repr)
ALL4 = sorted([(c, a) for c in ("Final", "Integrated") for a in ("Discrete", "Continuous")], key=repr)
FD = [("Final", "Discrete")]
BOTH = ["Continuous", "Discrete"]
S01 = [0, 1]


def _expected():
    e = {}
    # KDyn
    for N in (8, 16, 20, 28, 36, 6, 10, 22):
        e[("kdyn", N, "plain")] = ALL4 if N in (8, 10) else TWO
    for v in ("SMO_KD_ANY=1", "ckpt=3", "SMO_KD_DENSE_FROM=4", "SMO_KD_TYSTACK=0", "SMO_KD_FUSE_NEXT=0", "SMO_KD_GRAPH=0", "batch=3", "frozen_U",
              "devices=[0,0]"):
        e[("kdyn", 16, v)] = TWO
    for v in ("SMO_KD_TYPAD=24", "SMO_KD_TYL=0", "SMO_KD_ADJ_SEQ=0", "ckpt=3,SMO_KD_TYCACHE=0"):
        e[("kdyn", 16, v)] = TWO
    e[("kdyn", 16, "frozen_U,keep_states=False")] = FD           # (no stack: the Final cost only)
    e[("kdyn", 24, "graph")] = TWO
    e[("kdyn", 16, "gram")] = [("Final", None)]
    e[("kdyn", 16, "transform")] = e[("kdyn", 10, "transform")] = [("Final", None)]
    e[("kdyn", 128, "plain")] = e[("kdyn", 256, "plain")] = FD
    # SH23
    for N in (16, 21, 54, 64, 1100):
        e[("sh23", N, "plain")] = BOTH
    for N, v in ((64, "SMO_SH_ANY=1"), (54, "batch=3"), (64, "horizons"), (64, "a per member")):
        e[("sh23", N, v)] = BOTH
    e[("sh23", 54, "gram")] = [None]
    for N in (64, 54, 1024):                                         # Hessian-vector products: the discrete adjoint alone has them
        e[("sh23", N, "hessvec")] = ["Discrete"]
    e[("sh23", 64, "hessvec,horizons")] = ["Discrete"]
    # SHB23
    for N in (20, 64, 127, 256, 1023):
        e[("shb23", N, "plain")] = [None]
    for N, v in ((256, "SMO_SHB_CLUSTER=0"), (64, "SMO_SHB_ANY=1"), (32, "continuous"), (256, "continuous"), (64, "batch=3"), (512, "batch=3"),
                 (20, "transform"), (127, "transform")):
        e[("shb23", N, v)] = [None]
    # Poiseuille
    for sz in ((12, 12), (24, 24), (18, 15), (30, 66), (42, 27)):
        e[("pois", sz, "plain")] = S01
    for sz in ((16, 16), (32, 24)):
        e[("pois", sz, "continuous")] = S01
    for v in ("SMO_POIS_APPLY=dense", "SMO_POIS_XFFT=0", "SMO_POIS_XPROD=1", "SMO_POIS_HODLR_SPLIT=3", "ckpt=2", "batch=3,SMO_POIS_APPLY_MB=1",
              "batch=3,SMO_POIS_APPLY_MB=2", "batch=3,SMO_POIS_APPLY_MB=4"):
        e[("pois", (30, 66), v)] = S01
    e[("pois", (18, 15), "transform")] = [0]
    return e


def test_the_case_table_names_every_path_exactly_once():
    cov, want = po.coverage(), _expected()
    assert sorted(cov, key=repr) == sorted(want, key=repr)
    for key in want:
        assert cov[key] == want[key], key                            # (a repeated combination would show as a longer list)
    ids = [c["id"] for c in po.CASES]
    assert len(set(ids)) == len(ids) == sum(len(v) for v in want.values())


def test_the_cases_carry_what_their_name_says():
    by = {c["id"]: c for c in po.CASES}
    assert by["kdyn-16-ckpt=3-Final-Discrete"]["ckpt"] == 3 and by["kdyn-16-ckpt=3-Final-Discrete"]["n"] == 7
    dense = by["kdyn-16-SMO_KD_DENSE_FROM=4-Final-Discrete"]
    assert dense["ckpt"] == 2 and dense["n"] == 9 and dense["env"] == {"SMO_KD_DENSE_FROM": "4"}
    assert by["kdyn-24-graph-Final-Discrete"]["n"] == 8 and by["kdyn-24-graph-Final-Discrete"]["replays"]
    batch = by["kdyn-16-batch=3-Final-Discrete"]
    assert batch["batch"] == 3 and batch["hz"] == (3, 1, 2) and len(set(batch["rm"])) == 3
    assert by["kdyn-16-gram"]["batch"] == 3 and by["sh23-54-gram"]["batch"] == 3
    assert by["kdyn-16-devices=[0,0]-Final-Discrete"]["devices"] == (0, 0)
    assert all(by["kdyn-%d-Final-Discrete" % N]["n"] == 2 for N in (128, 256))
    assert by["sh23-64-horizons-Discrete"]["hz"] == (4, 2, 3) and len(set(by["sh23-64-a_per_member-Discrete"]["a"])) == 3
    assert by["pois-30x66-ckpt=2-s1"]["ckpt"] == 2
    nocache = by["kdyn-16-ckpt=3,SMO_KD_TYCACHE=0-Final-Discrete"]
    assert nocache["ckpt"] == 3 and nocache["n"] == 7 and nocache["env"] == {"SMO_KD_TYCACHE": "0"}
    assert by["kdyn-16-SMO_KD_TYPAD=24-Final-Discrete"]["env"] == {"SMO_KD_TYPAD": "24"}
    assert by["kdyn-16-SMO_KD_TYL=0-Final-Discrete"]["env"] == {"SMO_KD_TYL": "0"}
    assert by["kdyn-16-SMO_KD_ADJ_SEQ=0-Final-Discrete"]["env"] == {"SMO_KD_ADJ_SEQ": "0"}
    assert all(by["sh23-%d-hessvec-Discrete" % N]["hessvec"] for N in (64, 54, 1024))
    hv = by["sh23-64-hessvec,horizons-Discrete"]
    assert hv["hessvec"] and hv["batch"] == 3 and hv["hz"] == (4, 2, 3)
    assert [c["id"] for c in po.CASES if c.get("hessvec")] == ["sh23-64-hessvec-Discrete", "sh23-54-hessvec-Discrete", "sh23-1024-hessvec-Discrete",
                                                               "sh23-64-hessvec,horizons-Discrete"]
    for c in po.CASES:
        for name, value in c["env"].items():
            assert "%s=%s" % (name, value) in c["variant"], c["id"]
        if c["family"] == "kdyn" and c["variant"] == "plain" and c["size"] < 128:
            assert c["n"] == 3
        if c["family"] == "pois" and c.get("op") is None:
            assert c["n"] == 3
    assert po.FILLS == (None, 0x00, 0xFF, 0x3F) and po.VEC_SIZES == (1, 7, 1001)
    assert po.fill_pattern(0x3F, 2).view("u8").tolist() == [0x3F3F3F3F3F3F3F3F] * 2 and 4.7e-4 < po.fill_pattern(0x3F, 1)[0] < 4.8e-4
    assert po.fill_pattern(0xFF, 1)[0] != po.fill_pattern(0xFF, 1)[0]           # a NaN


def test_poison_ops_imports_without_the_library():
    code = ("import sys, poison_ops; bad = [m for m in sys.modules if m.split('.')[0] in ('spheremanopt_amd', 'oracle', 'torch')]; "
            "assert not bad, bad; print(len(poison_ops.CASES))")
    import os
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == len(po.CASES)
