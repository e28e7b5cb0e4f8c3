"""bench.py's output contract (one JSON line on stdout; the fields the driver and the judge read), exercised end to end on the
GPU with short runs: the pipelined schedule, and under --full the roofline leg (HIP events per launch) and the CPU-baseline leg."""
import glob
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(flags), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines                      # exactly one line on stdout
    return json.loads(lines[0])


def test_bench_json_line_contract():
    d = _run("--steps", "4", "--warmup", "2", "--full")
    assert d["metric"].startswith("scenes/s fwd+bwd KITTI-Car bs=2/GPU") and d["unit"] == "scenes/s"
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and d["dtype"] == "f32"
    assert d["value"] > 50 and abs(d["value"] - 2 * 1000.0 / d["ms_per_step"]) < 0.01 * d["value"]      # bs = 2 scenes per step
    cfg = d["config"]
    assert "workload" in cfg and "model" not in cfg and cfg["global_batch"] == 2 and cfg["parallelism"] == "dp1"
    # the workload is fixed: every step draws unseen scenes (no recycled batches for the optimizer to memorise); level rows are reported
    assert cfg["distinct_batches"] >= 64 + 4 + 1 and cfg["priming_steps"] == 62
    lv = cfg["level_rows"]
    assert lv["det_L0"]["median"] >= lv["det_voxels"]["median"] > 5000 and lv["det_L1"]["min"] > 1000 and lv["occ_out"]["median"] > 50000
    assert lv["det_voxels_after_pass_occ"]["median"] >= lv["det_voxels"]["median"]
    assert cfg["recurring_batches_scenes_per_s"]["scenes_per_s"] > 50
    r = d["roofline"]
    assert (r["traffic"] is None) == (r["traffic_source"] is None)
    # "latency": neither roof within a factor 5 (frac_hbm_measured and frac_mfma < 0.2); the fraction is still quoted against the HBM roof
    assert r["bound"] in ("hbm", "mfma", "latency") and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4 and 0.05 < r["frac"] < 1.0
    assert r["traffic"] is None or r["traffic"] > 1e6
    assert r["launches_per_step"] == 54.0 and 10 < r["avg_launch_us"] < 500
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and c["unit"] == "scenes/s" and "sample" in c
    assert d["rulebook_hbm_GBps"] > 1


def test_bench_plain_run_times_the_headline_and_dumps_outputs(tmp_path):
    """without --full: the headline measurement only (no secondary legs), and --dump-outputs writes the last timed step's loss and the
    trained model's floating-point state as float32 .npy files, 64 MB at most -- the same bits in a second run with the same arguments"""
    out = tmp_path / "outputs"
    d = _run("--steps", "3", "--warmup", "1", "--dump-outputs", str(out))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "scenes/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 50 and abs(d["value"] - 2 * 1000.0 / d["ms_per_step"]) < 0.01 * d["value"]
    assert d["config"]["priming_steps"] == 63 and d["config"]["level_rows"]["det_voxels"]["median"] > 5000
    for k in ("roofline", "cpu_baseline", "other_kernels", "rulebook_hbm_GBps"):
        assert k not in d, k
    for k in ("in_order_scenes_per_s", "recurring_batches_scenes_per_s", "with_rpn_heads", "with_all_heads", "predicted_scaling_eff"):
        assert k not in d["config"], k
    import numpy as np
    files = sorted(glob.glob(str(out / "*.npy")))
    names = [os.path.basename(f)[:-4] for f in files]
    assert "loss" in names and "state.det_modules.backbone_3d.conv_out.0.weight" in names and len(names) > 100
    assert sum(os.path.getsize(f) for f in files) <= 64 * 2 ** 20
    loss = np.load(str(out / "loss.npy"))
    assert loss.dtype == np.float32 and loss.size == 1 and np.isfinite(loss).all() and (loss > 0).all()
    for f in files:
        a = np.load(f)
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
    # bit for bit over the ~66 training steps: every reduction on the path is order-independent except the fused BatchNorm statistics,
    # whose per-slot fp64 sums take atomic adds from several workgroups (bn_fuse.h, conv_apply_split.hip).  Those sums reach the model
    # only rounded to fp32 (mean, rstd), so their order shows only when an fp64 sum lies within its last bits of an fp32 rounding
    # boundary: rare, but if this fails once and passes on a rerun, that is where to look.
    again = tmp_path / "again"
    _run("--steps", "3", "--warmup", "1", "--dump-outputs", str(again))
    assert sorted(os.listdir(str(again))) == sorted(os.path.basename(f) for f in files)
    for f in files:
        np.testing.assert_array_equal(np.load(f), np.load(str(again / os.path.basename(f))), err_msg=f)


def test_bench_in_order_schedule_still_runs():
    """BTC_SCHEDULE=in_order: no worker thread, no side-stream preparation -- the plain step the roofline leg uses"""
    env = dict(os.environ, BTC_SCHEDULE="in_order")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-roofline"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.strip()][-1])
    assert d["value"] > 50 and d["config"]["schedule"].startswith("in order, one stream")


def test_bench_distributed_path_at_world_size_one():
    """BTC_BENCH_FORCE_DIST=1: process group over RCCL, bucketed reducer, barriers and max-over-ranks timing at world size 1 -- the code
    path the driver's N > 1 launches take, on the one GPU a test box has (--priming: fewer optimizer steps before the timed region)"""
    env = dict(os.environ, BTC_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--priming", "8", "--no-cpu-baseline",
                        "--no-roofline", "--no-extras"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines                      # RCCL's banner went to stderr
    d = json.loads(lines[0])
    assert d["value"] > 50 and d["n_gpus"] == 1 and d["config"]["priming_steps"] == 7
    assert d["config"]["collective"]["backend"] == "nccl" and d["config"]["collective"]["world_size"] == 1
