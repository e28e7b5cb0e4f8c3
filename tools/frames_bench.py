#!/usr/bin/env python3
"""KITTI frames into a resident batch: the per-scene host crop + upload against KittiFrames.load_batch, alternating in ONE process.

A synthetic KITTI directory at the real shape: batch size 2, --rows rows per scan (a Velodyne HDL-64 scan has about 120 K) drawn all
around the sensor out to 70 m, KITTI-like calibrations and image shapes.  The kept share that this geometry produces is reported; a real
scan's share depends on the scene.  The files are written once and then served from the page cache: disk time is in neither route.

  host     per scene np.fromfile + Calibration.lidar_to_rect + get_fov_flag + boolean index (the reference's numpy statements,
           KittiFrames.fov_crop_host), then the upload of the cropped points and the scene offsets;
  device   KittiFrames.load_batch: the files read into one pinned buffer, one upload, btc_fov_crop, the (B+1)-int read-back;
  kernels  btc_fov_crop alone on a batch that is already on the device, between two device events.

`host` is THE BASELINE, not code under test.  Host clock around --batches batches ending in a device synchronisation, `host` and
`device` alternating --alternations times.  Writes profiles/frames_bench.json.
"""
import argparse
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--scene-batches", type=int, default=4, help="distinct scene batches, cycled")
    ap.add_argument("--rows", type=int, default=120000, help="rows per raw scan")
    ap.add_argument("--alternations", type=int, default=5, help="timed blocks PER PATH (at least 5 for a result that is reported)")
    ap.add_argument("--batches", type=int, default=50, help="batches per timed block (at least 50 for a result that is reported)")
    ap.add_argument("--kernel-calls", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    return ap.parse_args(argv)


def make_directory(root, n_frames, rows, seed=11):
    """velodyne / calib / infos of n_frames frames in the reference's on-disk formats; the calibrations are those of the test fixture"""
    import numpy as np
    import kitti_frames_ref as kr
    for sub in ("training/velodyne", "training/calib", "ImageSets"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    rng = np.random.default_rng(seed)
    infos = []
    for i in range(n_frames):
        fid = "%06d" % i
        n = int(rows * rng.uniform(0.95, 1.05))
        r, az = rng.uniform(2.0, 70.0, n), rng.uniform(-np.pi, np.pi, n)
        pts = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-2.5, 1.0, n), rng.uniform(0, 1, n)], axis=1).astype(np.float32)
        pts.tofile(os.path.join(root, "training/velodyne/%s.bin" % fid))
        with open(os.path.join(root, "training/calib/%s.txt" % fid), "w") as f:
            f.write(kr.calib_text(kr.calib_arrays(i % kr.N_FRAMES)))
        infos.append({"point_cloud": {"num_features": 4, "lidar_idx": fid},
                      "image": {"image_idx": fid, "image_shape": np.array(kr.IMAGE_SHAPES[i % kr.N_FRAMES], np.int32)}})
    with open(os.path.join(root, "kitti_infos_train.pkl"), "wb") as f:
        pickle.dump(infos, f)
    with open(os.path.join(root, "ImageSets/train.txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in range(n_frames)))


def measure(args, device, root):
    import numpy as np
    import torch
    from btcdet_amd._lib import lib, ptr, stream_ptr, workspace
    from btcdet_amd.kitti_frames import KittiFrames
    t0 = time.perf_counter()
    B = args.batch_size
    make_directory(root, args.scene_batches * B, args.rows)
    frames = KittiFrames(root, "train")
    batches = [list(range(k * B, (k + 1) * B)) for k in range(args.scene_batches)]
    setup_s = time.perf_counter() - t0

    def host(idx):
        res = [frames.fov_crop_host(i) for i in idx]
        pts = torch.from_numpy(np.concatenate(res)).to(device)
        offs = torch.from_numpy(np.cumsum([0] + [r.shape[0] for r in res]).astype(np.int32)).to(device)
        return pts, offs

    def dev(idx):
        b = frames.load_batch(idx, device)
        return b["points"], b["scene_offsets"]

    fns = {"host": host, "device": dev}
    # The device route makes the decisions of the header's formulas (checked here against their numpy restatement, row for row); the
    # host route's np.dot goes through BLAS, so a point within rounding of an image edge may be decided differently: counted, reported.
    import kitti_frames_ref as kr
    from btcdet_amd.kitti_frames import calib_block, get_fov_flag
    differ = 0
    for idx in batches:
        dp, do = dev(idx)
        bounds, got = do.tolist(), dp.cpu().numpy()
        for b, i in enumerate(idx):
            scan = np.fromfile(str(frames.lidar_path(i)), dtype=np.float32).reshape(-1, 4)
            keep = kr.restate_keep(scan, calib_block(frames.calib(i), frames.image_shape(i)))
            assert got[bounds[b]:bounds[b + 1]].tobytes() == scan[keep].tobytes(), "btc_fov_crop differs from the restatement of its header"
            with np.errstate(all="ignore"):
                differ += int((keep != get_fov_flag(frames.calib(i).lidar_to_rect(scan[:, 0:3]), frames.image_shape(i), frames.calib(i))).sum())

    def block(mode, n, start):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(n):
            fns[mode](batches[(start + i) % len(batches)])
        torch.cuda.synchronize()      # inside the host clock
        return (time.perf_counter() - t) / n * 1e6

    raw = [frames.load_batch(idx, device, crop=False) for idx in batches]
    kept = [frames.load_batch(idx, device)["points"].shape[0] for idx in batches]
    res = {"batch_size": B, "rows_per_batch": [int(r["points"].shape[0]) for r in raw], "kept_rows_per_batch": kept,
           "kept_share": round(sum(kept) / sum(int(r["points"].shape[0]) for r in raw), 4),
           "rows_the_blas_route_decides_differently": differ, "setup_s": round(setup_s, 1),
           "batches_per_block": args.batches, "us_per_batch": {"host": [], "device": []}}
    for m in fns:
        block(m, args.warmup, 0)
    for a in range(args.alternations):
        for m in fns:
            res["us_per_batch"][m].append(block(m, args.batches, a))
    # the kernels alone: one batch on the device, the entry point called back to back between two events
    pts, offs = raw[0]["points"], raw[0]["scene_offsets"]
    cal = torch.from_numpy(frames.calib_blocks(batches[0])).to(device)
    n, ld = pts.shape
    out = torch.empty_like(pts)
    new_offs = torch.empty((B + 1,), dtype=torch.int32, device=device)
    ws_bytes = lib().btc_fov_crop_ws_bytes(n, B)
    ws = workspace(ws_bytes, device)

    def kernels(calls):
        for _ in range(calls):
            rc = lib().btc_fov_crop(ptr(pts), n, ld, ptr(offs), B, ptr(cal), n, ptr(out), ptr(new_offs), None, ptr(ws), ws_bytes, stream_ptr())
            assert rc == 0
    kernels(20)
    res["kernels_us_per_batch"] = []
    for a in range(args.alternations):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        kernels(args.kernel_calls)
        e1.record()
        torch.cuda.synchronize()
        res["kernels_us_per_batch"].append(e0.elapsed_time(e1) * 1e3 / args.kernel_calls)
    res["us_per_batch_median"] = {m: statistics.median(v) for m, v in res["us_per_batch"].items()}
    res["us_per_batch_spread"] = {m: max(v) - min(v) for m, v in res["us_per_batch"].items()}
    res["kernels_us_per_batch_median"] = statistics.median(res["kernels_us_per_batch"])
    med, spr = res["us_per_batch_median"], res["us_per_batch_spread"]
    res["scenes_per_s"] = {m: B / med[m] * 1e6 for m in med}
    res["device_below_host_by_more_than_host_spread"] = bool(med["host"] - med["device"] > spr["host"])
    return res


def main(argv=None):
    args = parse_args(argv)
    import torch
    import infer_bench
    assert torch.cuda.is_available(), "tools/frames_bench.py needs a GPU"
    with tempfile.TemporaryDirectory() as d:
        out = {"head": infer_bench.head_commit(), "alternations": args.alternations, "frames": measure(args, torch.device("cuda:0"), d)}
    print(json.dumps(out["frames"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
