"""bench.py logic that needs no GPU: `--gpus N` starts the ranks itself before anything touches a GPU, a world size other than N is
refused, and PMC traffic is quoted only from a counter summary collected from exactly the kernel sources of this tree."""
import importlib.util
import json
import os
import subprocess
import sys

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_gpus_flag_spawns_ranks_without_touching_a_gpu():
    """Here there is no GPU: both child ranks must come up (torch.distributed.run) and each refuse with the no-GPU message; the parent
    only forwards their exit status.  A parent that ignored --gpus would print ONE such message, from itself."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--npts", "16", "--iters", "2"], capture_output=True,
                       text=True, env=env, timeout=300)
    assert p.returncode != 0
    assert p.stderr.count("bench.py needs a GPU") == 2, p.stderr[-2000:]
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_world_size_mismatch_is_refused_before_any_gpu_work():
    env = dict(os.environ, PYTHONPATH=ROOT, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode != 0 and "--gpus 8" in p.stderr and "2 rank" in p.stderr


def test_full_is_off_by_default(monkeypatch):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = b.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = b.parse()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_keeps_small_vectors_and_samples_large_ones(tmp_path):
    """--dump-outputs: float64 .npy files; a vector above DUMP_SAMPLE entries becomes a sample at fixed seeded indices plus its norm, the
    same from call to call; all of a run's files stay under 64 MB; N ranks write their parts under a _rank<r> suffix."""
    import argparse
    import numpy as np
    b = _bench()
    a = argparse.Namespace(dump_outputs=None)
    b.keep_outputs(a, J=1.0)
    assert not hasattr(a, "outputs")                                           # no --dump-outputs: nothing is kept
    big = np.arange(3 * 10 ** 6, dtype=np.float64)
    for sub in ("one", "two"):
        a = argparse.Namespace(dump_outputs=str(tmp_path / sub))
        b.keep_outputs(a, J=-8.5e-6, grad_B=big, grad_U=np.float32(2) * np.ones(1000, dtype=np.float32))
        b.write_outputs(a)
    d = {f.name[:-4]: np.load(f) for f in (tmp_path / "one").iterdir()}
    assert sorted(d) == ["J", "grad_B_norm", "grad_B_sample", "grad_U"] and all(v.dtype == np.float64 for v in d.values())
    assert d["J"].tolist() == [-8.5e-6] and d["grad_U"].tolist() == [2.0] * 1000
    s = d["grad_B_sample"]                                                     # big[i] == i: the sample shows its indices
    assert s.size == b.DUMP_SAMPLE and np.all(np.diff(s) >= 0) and s[0] >= 0 and s[-1] < big.size and len(np.unique(s)) > 0.8 * s.size
    assert d["grad_B_norm"].tolist() == [np.linalg.norm(big)]
    for k, v in d.items():
        assert np.array_equal(np.load(tmp_path / "two" / (k + ".npy")), v), k
    assert sum(f.stat().st_size for f in (tmp_path / "one").iterdir()) < 64 * 2 ** 20
    a = argparse.Namespace(dump_outputs=str(tmp_path / "ranks"))
    b.keep_outputs(a, rank=1, world=4, J=3.0, grad_B=big)
    b.write_outputs(a)
    assert sorted(f.name for f in (tmp_path / "ranks").iterdir()) == ["J_rank1.npy", "grad_B_norm_rank1.npy", "grad_B_sample_rank1.npy"]
    assert np.load(tmp_path / "ranks" / "grad_B_sample_rank1.npy").size == b.DUMP_SAMPLE // 4


def test_pmc_traffic_is_tied_to_the_kernel_sources(tmp_path, monkeypatch):
    b = _bench()
    sha = b.source_sha()
    assert len(sha) == 16 and sha == b.source_sha()
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(b, "ROOT", str(tmp_path))
    monkeypatch.setattr(b, "source_sha", lambda: sha)
    val, src = b.pmc_traffic("kd_x_pass<fused_adj>", 128)
    assert val is None and "reason" in src
    rec = {"source_sha": "0" * 16, "kernels": {"kd_x_pass<fused_adj>": {"hbm_bytes_per_launch": 1.0, "instantiation": "x"}}}
    (prof / "r07_kdyn128_pmc.json").write_text(json.dumps(rec))
    assert b.pmc_traffic("kd_x_pass<fused_adj>", 128)[0] is None              # another build's counters are not quoted
    rec["source_sha"] = sha
    rec["kernels"]["kd_x_pass<fused_adj>"]["hbm_bytes_per_launch"] = 7.5e8
    (prof / "r08_kdyn128_pmc.json").write_text(json.dumps(rec))
    val, src = b.pmc_traffic("kd_x_pass<fused_adj>", 128)
    assert val == 7.5e8 and src["file"].endswith("r08_kdyn128_pmc.json") and src["source_sha"] == sha
    assert b.pmc_traffic("kd_x_pass<fused_adj>", 256)[0] is None               # other grid: other file
    assert b.pmc_traffic("kd_y_pass<inv>", 128)[0] is None                     # kernel not in the summary


def test_committed_pmc_summaries_match_this_tree():
    """The summaries under profiles/ that bench.py would quote must have been collected from the kernel sources as committed — rerun
    tools/profile_round.sh (and copy its pmc_<N>.json) after changing anything under spheremanopt_amd/csrc/."""
    import warnings
    b = _bench()
    for n in (128, 256):
        val, src = b.pmc_traffic("kd_x_pass<fused_adj>", n)
        if val is None:                       # not an error of the code: bench.py then reports traffic = null, as it must
            warnings.warn("profiles/ holds no PMC summary of the current kernel sources for %d^3: %s" % (n, src["reason"]))
        else:
            assert val > 0 and src["source_sha"] == b.source_sha()
