#!/usr/bin/env python3
"""The ground-truth database: the host route to a resident ObjectBank against GtDatabase.build, alternating in ONE process.

A synthetic KITTI directory at the real shape: --frames frames of --rows rows per scan (a Velodyne HDL-64 scan has about 120 K) drawn
all around the sensor, --boxes boxes per frame with a cluster of rows inside each.  The files are written once and then served from the
page cache: disk reads of the scans are in neither route.

  host     per frame np.fromfile + database_sampler.points_in_boxes_mask + boolean index + the centre subtraction + one .bin written
           per object (the reference's statements, with the project's numpy predicate in place of the compiled op), the db_infos, then
           ObjectBank(root, db_infos) reading the files back and .tensor(device);
  device   GtDatabase.build(frames, frames_per_batch): the scans up in one copy per batch, btc_cut_objects, a bank that is resident;
  kernels  btc_cut_objects alone (five launches) on batches of --kernel-frames frames that are already on the device, between two device
           events, with the bytes the algorithm needs (the scan read twice, the cut rows written once) over that time.

`host` is THE BASELINE, not code under test.  Host clock around one whole database ending in a device synchronisation, `host` and
`device` alternating --alternations times.  Writes profiles/gt_database_bench.json.
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
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--frames-per-batch", type=int, default=16)
    ap.add_argument("--rows", type=int, default=120000, help="rows per raw scan")
    ap.add_argument("--boxes", type=int, default=6, help="boxes per frame (KITTI train: 14 357 objects of the three classes in 3 712 frames, and DontCare)")
    ap.add_argument("--cluster", type=int, default=300, help="rows drawn inside each box")
    ap.add_argument("--alternations", type=int, default=5, help="timed blocks PER PATH (at least 5 for a result that is reported)")
    ap.add_argument("--kernel-calls", type=int, default=50)
    ap.add_argument("--kernel-frames", type=int, nargs="*", default=[2, 16, 64], help="batch sizes at which the kernels alone are timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_database_bench.json"))
    return ap.parse_args(argv)


def make_directory(root, args, seed=13):
    import numpy as np
    import kitti_frames_ref as kr
    for sub in ("training/velodyne", "training/calib", "ImageSets"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    rng = np.random.default_rng(seed)
    infos = []
    for i in range(args.frames):
        fid = "%06d" % i
        m = args.boxes
        boxes = np.stack([rng.uniform(5, 60, m), rng.uniform(-25, 25, m), rng.uniform(-1.2, -0.4, m), rng.uniform(3.2, 4.6, m), rng.uniform(1.5, 1.9, m),
                          rng.uniform(1.4, 1.9, m), rng.uniform(-3.1, 3.1, m)], axis=1)
        n = int(args.rows * rng.uniform(0.95, 1.05))
        r, az = rng.uniform(2.0, 70.0, n), rng.uniform(-np.pi, np.pi, n)
        pts = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-2.5, 1.0, n), rng.uniform(0, 1, n)], axis=1)
        b = boxes[rng.integers(0, m, m * args.cluster)]
        loc = rng.uniform(-1.0, 1.0, (b.shape[0], 3)) * (b[:, 3:6] / 2)
        c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
        near = np.stack([b[:, 0] + loc[:, 0] * c - loc[:, 1] * s, b[:, 1] + loc[:, 0] * s + loc[:, 1] * c, b[:, 2] + loc[:, 2], rng.uniform(0, 1, b.shape[0])], axis=1)
        pts = np.concatenate([pts, near])[rng.permutation(n + near.shape[0])].astype(np.float32)
        pts.tofile(os.path.join(root, "training/velodyne/%s.bin" % fid))
        with open(os.path.join(root, "training/calib/%s.txt" % fid), "w") as f:
            f.write(kr.calib_text(kr.calib_arrays(i % kr.N_FRAMES)))
        annos = {"name": np.array(["Car"] * m + ["DontCare"]), "difficulty": np.zeros(m + 1, np.int32), "bbox": np.zeros((m + 1, 4), np.float32),
                 "score": -np.ones(m + 1), "gt_boxes_lidar": boxes}
        infos.append({"point_cloud": {"num_features": 4, "lidar_idx": fid},
                      "image": {"image_idx": fid, "image_shape": np.array(kr.IMAGE_SHAPES[i % kr.N_FRAMES], np.int32)}, "annos": annos})
    with open(os.path.join(root, "kitti_infos_train.pkl"), "wb") as f:
        pickle.dump(infos, f)
    with open(os.path.join(root, "ImageSets/train.txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in range(args.frames)))


def measure(args, device, root):
    import numpy as np
    import torch
    from btcdet_amd._lib import lib, ptr, stream_ptr, workspace
    from btcdet_amd.database_sampler import points_in_boxes_mask
    from btcdet_amd.device_augmentor import ObjectBank
    from btcdet_amd.gt_database import GtDatabase, cut_layout
    from btcdet_amd.kitti_frames import KittiFrames
    t0 = time.perf_counter()
    make_directory(root, args)
    frames = KittiFrames(root, "train", fov_points_only=False)
    setup_s = time.perf_counter() - t0
    host_root = os.path.join(root, "host_db")

    def host():
        os.makedirs(os.path.join(host_root, "gt_database"), exist_ok=True)
        db_infos = {}
        for k in range(len(frames)):
            info = frames.infos[k]
            fid, annos = info["point_cloud"]["lidar_idx"], info["annos"]
            points = np.fromfile(str(frames.lidar_path(k)), dtype=np.float32).reshape(-1, 4)
            gt_boxes = annos["gt_boxes_lidar"]
            mask = points_in_boxes_mask(points[:, 0:3], gt_boxes.astype(np.float32))
            for i in range(gt_boxes.shape[0]):
                rel = "gt_database/%s_%s_%d.bin" % (fid, annos["name"][i], i)
                gt_points = points[mask[i]]
                gt_points[:, :3] -= gt_boxes[i, :3]
                with open(os.path.join(host_root, rel), "w") as f:
                    gt_points.tofile(f)
                db_infos.setdefault(annos["name"][i], []).append(
                    {"name": annos["name"][i], "path": rel, "image_idx": fid, "gt_idx": i, "box3d_lidar": gt_boxes[i], "num_points_in_gt": gt_points.shape[0],
                     "difficulty": annos["difficulty"][i], "bbox": annos["bbox"][i], "score": annos["score"][i]})
        bank = ObjectBank(host_root, db_infos, 4)
        return bank.tensor(device), bank.table, db_infos

    def dev():
        db = GtDatabase.build(frames, frames_per_batch=args.frames_per_batch, device=device)
        return db.bank.tensor(device), db.bank.table, db.db_infos

    # both routes give the same database: per path the same bytes (the device route is held to the numpy predicate bit for bit)
    ht, htab, hinfos = host()
    dt, dtab, dinfos = dev()
    ha, da = ht.cpu().numpy(), dt.cpu().numpy()
    assert sorted(htab) == sorted(dtab)
    for path, (f0, n0) in htab.items():
        f1, n1 = dtab[path]
        assert n0 == n1 and ha[f0:f0 + n0].tobytes() == da[f1:f1 + n1].tobytes(), path
    fns = {"host": host, "device": dev}

    def block(mode):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fns[mode]()
        torch.cuda.synchronize()      # inside the host clock
        return time.perf_counter() - t

    res = {"frames": len(frames), "frames_per_batch": args.frames_per_batch, "rows_per_frame": args.rows + args.boxes * args.cluster,
           "boxes_per_frame": args.boxes, "objects": len(dtab), "object_rows": int(da.shape[0]), "setup_s": round(setup_s, 1),
           "s_per_database": {"host": [], "device": []}}
    for a in range(args.alternations):
        for m in fns:
            res["s_per_database"][m].append(block(m))
    # the kernels alone: one batch on the device, the entry point called back to back between two events, per batch size
    res["kernels"] = []
    for kf in args.kernel_frames:
        if kf > len(frames):
            continue
        idx = list(range(kf))
        raw = frames.load_batch(idx, device, crop=False)
        pts = raw["points"]
        lay = cut_layout(np.concatenate([[0], np.cumsum(raw["raw_rows"])]), [frames.infos[k]["annos"]["gt_boxes_lidar"] for k in idx])
        t = {k: torch.from_numpy(np.ascontiguousarray(lay[k])).to(device) for k in ("rows", "centre", "box_offsets", "scene_offsets")}
        n, ld = pts.shape
        B, m, mb = len(idx), lay["m"], lay["max_boxes"]
        out = torch.empty_like(pts)
        obj_offs = torch.empty((m + 1,), dtype=torch.int32, device=device)
        ws_bytes = lib().btc_cut_objects_ws_bytes(n, B, m, mb)
        ws = workspace(ws_bytes, device)

        def kernels(calls):
            for _ in range(calls):
                rc = lib().btc_cut_objects(ptr(pts), n, ld, ptr(t["scene_offsets"]), B, ptr(t["rows"]), ptr(t["centre"]), ptr(t["box_offsets"]), m, mb, n,
                                           ptr(out), ptr(obj_offs), None, ptr(ws), ws_bytes, stream_ptr())
                assert rc == 0
        kernels(5)
        us = []
        for a in range(args.alternations):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            kernels(args.kernel_calls)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / args.kernel_calls)
        cut_rows = int(obj_offs[-1])
        # bytes the algorithm needs: the scan read by the count and by the scatter stage, every cut row written once
        need = 2 * n * ld * 4 + cut_rows * ld * 4
        res["kernels"].append({"frames": kf, "rows": n, "boxes": m, "cut_rows": cut_rows, "us_per_call": us, "us_per_call_median": statistics.median(us),
                               "needed_bytes": need, "needed_gbytes_per_s": round(need / statistics.median(us) / 1e3, 1)})
    med = {k: statistics.median(v) for k, v in res["s_per_database"].items()}
    res["s_per_database_median"] = med
    res["s_per_database_spread"] = {k: max(v) - min(v) for k, v in res["s_per_database"].items()}
    res["frames_per_s"] = {k: len(frames) / med[k] for k in med}
    res["device_below_host_by_more_than_host_spread"] = bool(med["host"] - med["device"] > res["s_per_database_spread"]["host"])
    return res


def main(argv=None):
    args = parse_args(argv)
    import torch
    import infer_bench
    assert torch.cuda.is_available(), "tools/gt_database_bench.py needs a GPU"
    with tempfile.TemporaryDirectory() as d:
        out = {"head": infer_bench.head_commit(), "alternations": args.alternations, "gt_database": measure(args, torch.device("cuda:0"), d)}
    print(json.dumps(out["gt_database"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
