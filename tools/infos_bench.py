#!/usr/bin/env python3
"""Creating the KITTI infos: the reference's formulation on the host against KittiInfoBuilder.get_infos and add_coverage, alternating in
ONE process.

A synthetic raw KITTI directory at the real shape: --frames frames of --rows rows per scan drawn all around the sensor, --boxes boxes
per frame in front of the camera with a cluster of rows inside each, label_2 text, calibrations and PNGs.  The files are written once
and then served from the page cache: disk reads are in neither route.

  host      per frame np.fromfile, the numpy FOV crop (lidar_to_rect, get_fov_flag, boolean index) and scipy's Delaunay in_hull per
            box: kitti_dataset.py:181-194, the reference's statements.  THE BASELINE, not code under test.
  device    KittiInfoBuilder.get_infos(frames_per_batch): labels and headers on the host, the scans up in one copy per batch,
            btc_count_in_boxes, one read-back per batch.
  coverage  host: per object the template pickle and the database .bin read back and get_coords in numpy (coverage_cells_host, the
            reference's chain); device: add_coverage from a resident TemplateBank and GtDatabase.bank.
  kernels   btc_count_in_boxes alone on batches of --kernel-frames frames already on the device, and btc_coverage_cells alone over every
            job, between two device events, with the bytes each needs over that time.

Host clock around one whole pass ending in a device synchronisation, the two routes alternating --alternations times.  Writes
profiles/infos_bench.json.
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
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--frames-per-batch", type=int, default=16)
    ap.add_argument("--rows", type=int, default=120000, help="rows per raw scan")
    ap.add_argument("--boxes", type=int, default=6, help="boxes per frame")
    ap.add_argument("--cluster", type=int, default=300, help="rows drawn inside each box")
    ap.add_argument("--template-rows", type=int, default=2000, help="rows per best-match template")
    ap.add_argument("--alternations", type=int, default=5, help="timed blocks PER PATH (at least 5 for a result that is reported)")
    ap.add_argument("--kernel-calls", type=int, default=50)
    ap.add_argument("--kernel-frames", type=int, nargs="*", default=[2, 16], help="batch sizes at which btc_count_in_boxes alone is timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infos_bench.json"))
    return ap.parse_args(argv)


def make_directory(root, args, seed=17):
    import numpy as np
    import kitti_frames_ref as kr
    import kitti_infos_ref as ir
    for sub in ("training/velodyne", "training/calib", "training/label_2", "training/image_2", "ImageSets"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    rng = np.random.default_rng(seed)
    for i in range(args.frames):
        fid, k = "%06d" % i, i % kr.N_FRAMES
        text = kr.calib_text(kr.calib_arrays(k))
        c = kr.parse_calib(text)
        M = kr.lidar_to_rect_matrix(c["R0"], c["Tr_velo2cam"]).astype(np.float64)
        m = args.boxes
        x = rng.uniform(8, 60, m)
        boxes = np.stack([x, rng.uniform(-0.5, 0.5, m) * x, rng.uniform(-1.2, -0.4, m), rng.uniform(3.2, 4.6, m), rng.uniform(1.5, 1.9, m),
                          rng.uniform(1.4, 1.9, m), rng.uniform(-3.1, 3.1, m)], axis=1)
        n = int(args.rows * rng.uniform(0.95, 1.05))
        r, az = rng.uniform(2.0, 70.0, n), rng.uniform(-np.pi, np.pi, n)
        pts = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-2.5, 1.0, n), rng.uniform(0, 1, n)], axis=1)
        b = boxes[rng.integers(0, m, m * args.cluster)]
        loc = rng.uniform(-1.0, 1.0, (b.shape[0], 3)) * (b[:, 3:6] / 2)
        cs, sn = np.cos(b[:, 6]), np.sin(b[:, 6])
        near = np.stack([b[:, 0] + loc[:, 0] * cs - loc[:, 1] * sn, b[:, 1] + loc[:, 0] * sn + loc[:, 1] * cs, b[:, 2] + loc[:, 2], rng.uniform(0, 1, b.shape[0])], axis=1)
        np.concatenate([pts, near])[rng.permutation(n + near.shape[0])].astype(np.float32).tofile(os.path.join(root, "training/velodyne/%s.bin" % fid))
        with open(os.path.join(root, "training/calib/%s.txt" % fid), "w") as f:
            f.write(text)
        lines = []
        for bx in boxes:
            cam = np.array([bx[0], bx[1], bx[2] - bx[5] / 2, 1.0]) @ M
            lines.append("Car 0.00 0 0.00 100.00 100.00 200.00 160.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (bx[5], bx[4], bx[3], cam[0], cam[1], cam[2], -bx[6] - np.pi / 2))
        lines.append("DontCare -1 -1 -10 500.00 150.00 560.00 180.00 -1 -1 -1 -1000 -1000 -1000 -10")
        with open(os.path.join(root, "training/label_2/%s.txt" % fid), "w") as f:
            f.write("\n".join(lines) + "\n")
        H, W = kr.IMAGE_SHAPES[k]
        with open(os.path.join(root, "training/image_2/%s.png" % fid), "wb") as f:
            f.write(ir.png_bytes(H, W))
    with open(os.path.join(root, "ImageSets/train.txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in range(args.frames)))


def corners_of(boxes):
    """box_utils.boxes_to_corners_3d in numpy, float64"""
    import numpy as np
    t = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, 1], [1, -1, 1], [-1, -1, 1], [-1, 1, 1]]) / 2
    c = boxes[:, None, 3:6] * t[None]
    cs, sn = np.cos(boxes[:, 6])[:, None], np.sin(boxes[:, 6])[:, None]
    return np.stack([c[:, :, 0] * cs - c[:, :, 1] * sn, c[:, :, 0] * sn + c[:, :, 1] * cs, c[:, :, 2]], axis=2) + boxes[:, None, 0:3]


def spread(v):
    return max(v) - min(v)


def measure(args, device, root):
    import numpy as np
    import torch
    from scipy.spatial import Delaunay
    from btcdet_amd._lib import lib, ptr, stream_ptr, workspace
    from btcdet_amd.device_augmentor import DeviceAugmentor, TemplateBank
    from btcdet_amd.gt_database import GtDatabase
    from btcdet_amd.kitti_frames import KittiFrames, get_fov_flag
    from btcdet_amd import kitti_infos as ki
    t0 = time.perf_counter()
    make_directory(root, args)
    builder = ki.KittiInfoBuilder(root, "train")
    plain = builder.get_infos(count_inside_pts=False)
    frames = KittiFrames(root, "train", fov_points_only=False, infos=plain)
    setup_s = time.perf_counter() - t0

    def host():
        out = []
        for k in range(len(frames)):
            info = plain[k]
            points = np.fromfile(str(frames.lidar_path(k)), dtype=np.float32).reshape(-1, 4)
            calib = frames.calib(k)
            pts_fov = points[get_fov_flag(calib.lidar_to_rect(points[:, 0:3]), info["image"]["image_shape"], calib)]
            boxes = info["annos"]["gt_boxes_lidar"]
            num = -np.ones(len(info["annos"]["name"]), dtype=np.int32)
            for j, corners in enumerate(corners_of(boxes)):
                num[j] = (Delaunay(corners).find_simplex(pts_fov[:, 0:3]) >= 0).sum()
            out.append(num)
        return out

    def dev():
        return [x["annos"]["num_points_in_gt"] for x in builder.get_infos(frames_per_batch=args.frames_per_batch, device=device)]

    h, d = host(), dev()
    differing = int(sum(int((a != b).sum()) for a, b in zip(h, d)))     # rows are drawn without a margin: a row within rounding of a face may differ
    fns = {"host": host, "device": dev}

    def block(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()      # inside the host clock
        return time.perf_counter() - t

    res = {"frames": len(frames), "frames_per_batch": args.frames_per_batch, "rows_per_frame": args.rows + args.boxes * args.cluster,
           "boxes_per_frame": args.boxes, "setup_s": round(setup_s, 1), "counts_that_differ_from_in_hull": differing,
           "points_in_gt_total": int(sum(int(x[x >= 0].sum()) for x in d)), "s_per_pass": {"host": [], "device": []}}
    for a in range(args.alternations):
        for m in fns:
            res["s_per_pass"][m].append(block(fns[m]))

    # ---- coverage: the database and the templates as files (host route) and as resident banks (device route)
    infos = builder.get_infos(frames_per_batch=args.frames_per_batch, device=device)
    db = GtDatabase.build(KittiFrames(root, "train", fov_points_only=False, infos=infos), frames_per_batch=args.frames_per_batch, device=device)
    db.save(root)
    rng = np.random.default_rng(5)
    arrays = {}
    os.makedirs(os.path.join(root, "bm_Car"), exist_ok=True)
    for info in infos:
        for i, name in enumerate(info["annos"]["name"]):
            if name == "Car":
                t = (rng.uniform(-0.55, 0.55, (args.template_rows, 3)) * info["annos"]["gt_boxes_lidar"][i, 3:6]).astype(np.float32)
                arrays[("Car", int(info["point_cloud"]["lidar_idx"]), i)] = t
                with open(os.path.join(root, "bm_Car", "%d_%d.pkl" % (int(info["point_cloud"]["lidar_idx"]), i)), "wb") as f:
                    pickle.dump(t, f)
    templates = TemplateBank.from_arrays(arrays)
    templates.tensor(device), db.bank.tensor(device)

    def cov_host():
        out = []
        for info in infos:
            fid, annos = info["point_cloud"]["lidar_idx"], info["annos"]
            for i, name in enumerate(annos["name"]):
                if name != "Car":
                    continue
                with open(os.path.join(root, "bm_Car", "%d_%d.pkl" % (int(fid), i)), "rb") as f:
                    bm = pickle.load(f).reshape([-1, 3]).astype(np.float32)
                obj = np.fromfile(os.path.join(root, "gt_database", "%s_%s_%d.bin" % (fid, name, i)), dtype=np.float32).reshape([-1, 4])
                uo, ub = ki.coverage_cells_host(bm, obj, annos["gt_boxes_lidar"][i])
                out.append(uo / max(1, ub))
        return out

    def cov_dev():
        ki.add_coverage(infos, db.bank, templates, "train", device=device)
        return [float(r) for info in infos for r, name in zip(info["annos"]["coverage_rates"].reshape(-1), info["annos"]["name"]) if name == "Car"]

    ch, cd = cov_host(), cov_dev()
    cov = {"objects": len(ch), "template_rows": args.template_rows, "rates_that_differ": int(sum(a != b for a, b in zip(ch, cd))),
           "s_per_pass": {"host": [], "device": []}}
    for a in range(args.alternations):
        for m, fn in (("host", cov_host), ("device", cov_dev)):
            cov["s_per_pass"][m].append(block(fn))
    res["coverage"] = cov

    # ---- the kernels alone, between two device events
    def timed(call):
        call(5)
        us = []
        for a in range(args.alternations):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            call(args.kernel_calls)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / args.kernel_calls)
        return us

    res["kernels"] = []
    for kf in args.kernel_frames:
        if kf > len(frames):
            continue
        idx = list(range(kf))
        raw = frames.load_batch(idx, device, crop=False)
        pts = raw["points"]
        boxes = [infos[k]["annos"]["gt_boxes_lidar"] for k in idx]
        rows = np.concatenate([ki.hull_rows(b) for b in boxes])
        box_offs = np.concatenate([[0], np.cumsum([b.shape[0] for b in boxes])]).astype(np.int32)
        offs = np.concatenate([[0], np.cumsum(raw["raw_rows"])]).astype(np.int32)
        d_rows, d_cal, d_boff, d_off = DeviceAugmentor._upload([rows, frames.calib_blocks(idx), box_offs, offs], device)
        n, ld, m = pts.shape[0], pts.shape[1], rows.shape[0]
        out = torch.empty((m + kf,), dtype=torch.int32, device=device)
        ws_bytes = lib().btc_count_in_boxes_ws_bytes(n, kf)
        ws = workspace(ws_bytes, device)

        def count(calls):
            for _ in range(calls):
                rc = lib().btc_count_in_boxes(ptr(pts), n, ld, ptr(d_off), kf, ptr(d_cal), ptr(d_rows), ptr(d_boff), m, ptr(out), out[m:].data_ptr(),
                                              ptr(ws), ws_bytes, stream_ptr())
                assert rc == 0
        us = timed(count)
        need = n * ld * 4      # every row read once; nothing is written per row
        res["kernels"].append({"entry": "btc_count_in_boxes", "frames": kf, "rows": n, "boxes": m, "us_per_call": us, "us_per_call_median": statistics.median(us),
                               "needed_bytes": need, "needed_gbytes_per_s": round(need / statistics.median(us) / 1e3, 1)})
    jobs, pose, _ = ki.coverage_jobs(infos, db.bank, templates, "train")
    d_jobs, d_pose = DeviceAugmentor._upload([jobs, pose], device)
    tr, orows = templates.tensor(device), db.bank.tensor(device)
    J, max_rows = jobs.shape[0], int(jobs[:, [1, 3]].max())
    out = torch.empty((3 * J,), dtype=torch.int32, device=device)
    ws_bytes = lib().btc_coverage_cells_ws_bytes(J, max_rows)
    ws = workspace(ws_bytes, device)

    def cells(calls):
        for _ in range(calls):
            rc = lib().btc_coverage_cells(ptr(tr), tr.shape[0], ptr(orows), orows.shape[0], orows.shape[1], ptr(d_jobs), ptr(d_pose), J, max_rows, ptr(out),
                                          out[2 * J:].data_ptr(), ptr(ws), ws_bytes, stream_ptr())
            assert rc == 0
    us = timed(cells)
    need = int(2 * jobs[:, 1].sum() * 12 + jobs[:, 3].sum() * orows.shape[1] * 4)      # the template read by two passes, the object by one
    res["kernels"].append({"entry": "btc_coverage_cells", "jobs": J, "template_rows": int(jobs[:, 1].sum()), "object_rows": int(jobs[:, 3].sum()),
                           "us_per_call": us, "us_per_call_median": statistics.median(us), "needed_bytes": need,
                           "needed_gbytes_per_s": round(need / statistics.median(us) / 1e3, 1)})
    for part in (res, cov):
        med = {k: statistics.median(v) for k, v in part["s_per_pass"].items()}
        part["s_per_pass_median"] = med
        part["s_per_pass_spread"] = {k: spread(v) for k, v in part["s_per_pass"].items()}
        part["device_below_host_by_more_than_host_spread"] = bool(med["host"] - med["device"] > part["s_per_pass_spread"]["host"])
    res["frames_per_s"] = {k: len(frames) / v for k, v in res["s_per_pass_median"].items()}
    return res


def main(argv=None):
    args = parse_args(argv)
    import torch
    import infer_bench
    assert torch.cuda.is_available(), "tools/infos_bench.py needs a GPU"
    with tempfile.TemporaryDirectory() as d:
        out = {"head": infer_bench.head_commit(), "alternations": args.alternations, "infos": measure(args, torch.device("cuda:0"), d)}
    print(json.dumps(out["infos"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
