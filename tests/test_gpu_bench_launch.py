"""The N > 1 launch of bench.py on the ONE GPU the test box has: `--gpus 2 --share-gpu` starts two ranks,
each with its own engine, model replica and chain on GPU 0 (RCCL refuses two ranks on one device, so the collectives run over the
gloo host group): rank logic, barriers, gather and the aggregate of the report are exercised with real device work every round.
Also the plain one-GPU run's `--dump-outputs`."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_two_ranks_sharing_the_gpu_produce_one_aggregate_line():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu", "--rows-per-group", "80", "--steps", "12", "--warmup", "20",
                        "--cpu-leapfrogs", "0", "--ess-tune", "0"], capture_output=True, text=True, env=env, timeout=560)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["chains"] == 2 and out["scaling"] == "weak"
    assert out["collective_backend"].startswith("gloo") and out["rccl_ranks"] == 0
    per = out["leapfrog_steps_per_sec_per_chain"]
    assert len(per) == 2 and all(x > 1000 for x in per)
    # the whole-job value: both chains' leapfrogs over the slower rank's time
    assert out["leapfrog_steps_per_sec"] <= sum(per) * (1 + 1e-9) and out["leapfrog_steps_per_sec"] >= max(per)
    assert out["roofline"]["launches_timed"] > 0 and "group-block" in out["schedule"]


@pytest.mark.timeout(900)
def test_eight_ranks_sharing_the_gpu_produce_one_aggregate_line():
    """The launch the driver's 8-GPU node will make, at its own world size (VERDICT r04 "next" 6a): eight ranks, each with its own
    engine, replica and chain -- here all on GPU 0 --, the gloo control plane, the agreed fall-back of the RCCL probe, eight result
    records gathered into one line; every rank reports how long its synthetic data and its engine took to set up."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--share-gpu", "--rows-per-group", "80", "--steps", "8", "--warmup", "12",
                        "--cpu-leapfrogs", "0", "--ess-tune", "0"], capture_output=True, text=True, env=env, timeout=860)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["config"]["chains"] == 8 and out["scaling"] == "weak"
    assert out["collective_backend"].startswith("gloo") and out["rccl_ranks"] == 0
    per = out["leapfrog_steps_per_sec_per_chain"]
    assert len(per) == 8 and all(x > 200 for x in per)
    assert max(per) <= out["leapfrog_steps_per_sec"] <= sum(per) * (1 + 1e-9)
    assert len(out["setup"]["data_s_per_rank"]) == 8 and all(0 < x < 120 for x in out["setup"]["engine_s_per_rank"])
    out_dir = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "bench_n8_shared.json"), "w") as fh:
            fh.write(lines[0] + "\n")


@pytest.mark.timeout(600)
def test_plain_run_dumps_the_same_last_draw_twice(tmp_path):
    """A plain one-GPU run (C2-S) with `--dump-outputs`: the last timed draw (n float64) and its statistics as .npy, and two runs with
    the same arguments write the same arrays -- what lets two builds be compared output for output."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows-per-group", "80", "--steps", "12", "--warmup", "20",
                            "--dump-outputs", str(d)], capture_output=True, text=True, env=env, timeout=280)
        assert r.returncode == 0, r.stderr[-3000:]
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        assert out["steps"] == 12 and out["ms_per_step"] > 0
        assert "cpu_baseline" not in out and out["ess_run"] is None
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert a["draw.npy"].shape == (10000,) and a["draw.npy"].dtype == np.float64 and np.isfinite(a["draw.npy"]).all()
    assert {"stat_tree_size.npy", "stat_model_logp.npy", "stat_energy.npy", "stat_step_size.npy"} <= set(a)
    assert a["stat_tree_size.npy"] >= 1 and all(np.isfinite(v).all() for v in a.values())
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
