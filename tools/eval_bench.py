"""KITTI AP evaluation on the GPU, timed (btcdet_amd/kitti_eval.py, csrc/kitti_eval.hip).

    python tools/eval_bench.py            ->  profiles/eval_bench.json

The KITTI val split's size in synthetic frames (3 769 frames, about 10 ground truths and 15 detections each, three classes; the seeded
generator below).  Reports the wall time of one get_official_eval_result on the GPU (the second of two calls; the
first pays the library load and the allocator), the GPU time of its three stages by HIP events (overlaps, pass A, pass B with the
similarity reduction) and the host time between them, and -- for context only, labelled as such -- the numpy restatement of
tests/kitti_eval_ref.py on the first 200 frames on the same box (left out, and said so, where the test tree is not installed).  No rate is promised; this records what was seen.

Each step runs in a child process under its own time limit (--limit seconds): the frames are generated once and handed over in a file.
"""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CLASSES = ["Car", "Pedestrian", "Cyclist"]
GT_NAMES = ["Car", "Car", "Car", "Pedestrian", "Pedestrian", "Cyclist", "Van", "Person_sitting", "DontCare", "Truck"]
SIZES = {"Car": (3.9, 1.56, 1.6), "Van": (5.0, 2.2, 1.9), "Pedestrian": (0.8, 1.75, 0.65), "Person_sitting": (0.8, 1.3, 0.6),
         "Cyclist": (1.76, 1.73, 0.6), "Truck": (10.0, 3.2, 2.6), "DontCare": (-1.0, -1.0, -1.0)}   # (l, h, w)


def make_frames(n_frames, seed=2024):
    """synthetic annotations: 4 .. 16 ground truths and 8 .. 22 detections per frame (10 and 15 on average); most detections are
    jittered copies of a ground truth, the rest false positives"""
    import numpy as np
    rng = np.random.default_rng(seed)

    def boxes(names):
        n = len(names)
        h = rng.uniform(15, 130, n)
        x1, y1 = rng.uniform(0, 1100, n), rng.uniform(100, 240, n)
        dims = np.array([SIZES[k] for k in names]).reshape(n, 3) * rng.uniform(0.85, 1.15, (n, 1))
        return {"name": np.array(names, dtype="<U16"), "bbox": np.stack([x1, y1, x1 + h * rng.uniform(0.4, 2.0, n), y1 + h], 1), "dimensions": dims,
                "location": np.stack([rng.uniform(-20, 20, n), rng.uniform(1.2, 2.0, n), rng.uniform(5, 60, n)], 1),
                "rotation_y": rng.uniform(-np.pi, np.pi, n), "alpha": rng.uniform(-np.pi, np.pi, n)}

    gt_annos, dt_annos = [], []
    for _ in range(n_frames):
        n_gt, n_dt = int(rng.integers(4, 17)), int(rng.integers(8, 23))
        gt = boxes([GT_NAMES[i] for i in rng.integers(0, len(GT_NAMES), n_gt)])
        gt.update(occluded=rng.integers(0, 4, n_gt).astype(float), truncated=np.where(rng.random(n_gt) < 0.3, rng.uniform(0, 0.6, n_gt), 0.0),
                  coverage_rates=rng.uniform(0, 1, n_gt))
        real = np.flatnonzero(gt["name"] != "DontCare")
        src = rng.choice(real, size=min(len(real), int(0.7 * n_dt)), replace=False) if len(real) else real
        dt = boxes([CLASSES[i] for i in rng.integers(0, 3, n_dt)])
        k = len(src)
        for key, jitter in (("bbox", 3.0), ("location", 0.08), ("rotation_y", 0.05), ("alpha", 0.3)):
            dt[key][:k] = gt[key][src] + rng.normal(0, jitter, gt[key][src].shape)
        dt["dimensions"][:k] = gt["dimensions"][src] * rng.uniform(0.96, 1.04, (k, 3))
        dt["name"][:k] = [nm if nm in CLASSES else CLASSES[0] for nm in gt["name"][src]]
        dt.update(score=rng.uniform(0.05, 1.0, n_dt), truncated=np.zeros(n_dt), occluded=np.zeros(n_dt))
        gt_annos.append(gt)
        dt_annos.append(dt)
    return gt_annos, dt_annos


def stage_gpu(case_file):
    import torch
    from btcdet_amd import kitti_eval as ke
    gt, dt = pickle.load(open(case_file, "rb"))
    walls = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res, ret, _ = ke.get_official_eval_result(gt, dt, CLASSES)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    timings = {}
    t0 = time.perf_counter()
    ds = ke.Dataset(gt, dt)
    t1 = time.perf_counter()
    ke.evaluate(ds, [0, 1, 2], [0, 1, 2], ke.official_min_overlaps([0, 1, 2]), 0, 3, ds.compute_aos, timings=timings)
    t2 = time.perf_counter()
    out = {"wall_ms_first_call": walls[0], "wall_ms": walls[1], "concatenate_ms": (t1 - t0) * 1e3, "evaluate_ms": (t2 - t1) * 1e3,
           "gpu_ms_by_events": timings, "frames": ds.F, "ground_truths": ds.NG, "detections": ds.ND, "pairs_per_metric": ds.P,
           "combinations": 3 * 3 * 3 * 2, "device": torch.cuda.get_device_name(0), "Car_3d/moderate_R40": float(ret["Car_3d/moderate_R40"])}
    print(json.dumps(out), flush=True)


def stage_numpy(case_file, frames):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import kitti_eval_ref as ref
    except ImportError:
        print(json.dumps({"what": "numpy restatement not run: tests/kitti_eval_ref.py is not installed"}), flush=True)
        return
    gt, dt = pickle.load(open(case_file, "rb"))
    gt, dt = gt[:frames], dt[:frames]
    t0 = time.perf_counter()
    _, ret, _ = ref.get_official_eval_result(gt, dt, CLASSES)
    out = {"what": "numpy float64 restatement (tests/kitti_eval_ref.py), single thread, same box, context only", "frames": len(gt),
           "wall_ms": (time.perf_counter() - t0) * 1e3}
    print(json.dumps(out), flush=True)


def child(args, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, timeout=limit, stdout=subprocess.PIPE, check=True)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--numpy-frames", type=int, default=200)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each child step, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.json"))
    ap.add_argument("--stage", choices=["gpu", "numpy"], help=argparse.SUPPRESS)
    ap.add_argument("--case", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.stage == "gpu":
        return stage_gpu(a.case)
    if a.stage == "numpy":
        return stage_numpy(a.case, a.numpy_frames)
    t0 = time.perf_counter()
    gt, dt = make_frames(a.frames)
    gen_s = time.perf_counter() - t0
    with tempfile.TemporaryDirectory() as d:
        case_file = os.path.join(d, "case.pkl")
        pickle.dump((gt, dt), open(case_file, "wb"))
        out = {"tool": "tools/eval_bench.py", "frames": a.frames, "classes": CLASSES, "generate_s": gen_s,
               "gpu": child(["--stage", "gpu", "--case", case_file], a.limit),
               "numpy_subset": child(["--stage", "numpy", "--case", case_file, "--numpy-frames", str(a.numpy_frames)], a.limit)}
    print(json.dumps(out), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
