#!/usr/bin/env python3
"""Training augmentation of a batch: the per-scene host chain against the resident device path, alternating in ONE process.

KITTI-Car shape, batch size 2, synth.make_scene scans, a synthetic ground-truth database sized like KITTI's car class (--db-objects
objects, some tens of MB of points), the model config's queue: gt_sampling -> random_world_flip -> random_world_scaling ->
random_world_rotation with SAVE_PRE_ROT.

  host     per scene DataAugmentor.forward on a copy of the raw scan (numpy, what a DataLoader worker runs), then the upload of its
           result: points, pre_rot_points, scene offsets, rot_z;
  device   DeviceAugmentor.plan + apply on the raw scans that are already resident: the (B+1)-int read-back included;
  kernels  btc_augment_batch alone with a plan that is already on the device, between two device events.

`host` is THE BASELINE, not code under test.  Both paths run the sampler's BEV IoU on the GPU (database_sampler, as shipped), draw from
the same global numpy RNG and read the same database files / bank.  Host clock around --batches batches ending in a device
synchronisation, `host` and `device` alternating --alternations times.  Writes profiles/augment_bench.json.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


class Cfg(dict):
    __getattr__ = dict.get
    __setattr__ = dict.__setitem__


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--scene-batches", type=int, default=4, help="distinct scene batches, cycled")
    ap.add_argument("--db-objects", type=int, default=14357, help="objects of the synthetic database (KITTI train split: 14 357 cars)")
    ap.add_argument("--alternations", type=int, default=5, help="timed blocks PER PATH (at least 5 for a result that is reported)")
    ap.add_argument("--batches", type=int, default=50, help="batches per timed block (at least 50 for a result that is reported)")
    ap.add_argument("--kernel-calls", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    return ap.parse_args(argv)


def make_database(root, n_objects, seed=5):
    """objects in the reference's on-disk format (one float32 .bin of box-centred points each + a db_infos dict); the point counts
    follow a long-tailed distribution with a mean near 150, like cars cut out of KITTI scans"""
    import numpy as np
    os.makedirs(os.path.join(root, "gt_database"), exist_ok=True)
    rng = np.random.default_rng(seed)
    counts = np.clip(rng.lognormal(4.3, 1.1, n_objects), 5, 2000).astype(np.int64)
    infos = []
    for i in range(n_objects):
        box = np.array([rng.uniform(5, 65), rng.uniform(-35, 35), rng.uniform(-1.2, -0.6), 3.9 * rng.uniform(0.9, 1.1), 1.6 * rng.uniform(0.9, 1.1),
                        1.56 * rng.uniform(0.9, 1.1), rng.uniform(-3.1, 3.1)], dtype=np.float32)
        n = int(counts[i])
        pts = np.concatenate([rng.uniform(-0.5, 0.5, (n, 3)) * box[3:6], rng.uniform(0, 1, (n, 1))], axis=1).astype(np.float32)
        rel = "gt_database/%06d_Car_%d.bin" % (i // 4, i % 4)
        pts.tofile(os.path.join(root, rel))
        infos.append({"name": "Car", "path": rel, "image_idx": "%06d" % (i // 4), "gt_idx": i % 4, "box3d_lidar": box, "num_points_in_gt": n,
                      "difficulty": int(rng.integers(0, 3)), "bbox": np.zeros(4, np.float32), "score": -1.0})
    return {"Car": infos}


def queue():
    return Cfg(DISABLE_AUG_LIST=["placeholder"], AUG_CONFIG_LIST=[
        Cfg(NAME="gt_sampling", PREPARE={"filter_by_min_points": ["Car:5"], "filter_by_difficulty": [-1]}, SAMPLE_GROUPS=["Car:15"],
            NUM_POINT_FEATURES=4, DATABASE_WITH_FAKELIDAR=False, REMOVE_EXTRA_WIDTH=[0.0, 0.0, 0.0], LIMIT_WHOLE_SCENE=False, USE_ROAD_PLANE=False),
        Cfg(NAME="random_world_flip", ALONG_AXIS_LIST=["x"]),
        Cfg(NAME="random_world_scaling", WORLD_SCALE_RANGE=[0.95, 1.05]),
        Cfg(NAME="random_world_rotation", WORLD_ROT_ANGLE=[-0.78539816, 0.78539816], SAVE_PRE_ROT=True)])


def measure(args, device, db_root):
    import numpy as np
    import torch
    from btcdet_amd import synth
    from btcdet_amd._lib import lib, ptr, stream_ptr, workspace
    from btcdet_amd.device_augmentor import AugPlan, DataAugmentor, DeviceAugmentor, ObjectBank
    t0 = time.perf_counter()
    infos = make_database(db_root, args.db_objects)
    bank = ObjectBank(db_root, infos, 4)
    bank.tensor(device)
    aug = DataAugmentor(db_root, queue(), ["Car"], db_infos=infos)
    dev_aug = DeviceAugmentor(aug, bank)
    batches = []
    for k in range(args.scene_batches):
        scenes = []
        for b in range(args.batch_size):
            s = synth.make_scene(7000 + 10 * k + b)
            n = s["gt_boxes"].shape[0]
            scenes.append({"points": s["points"], "gt_boxes": s["gt_boxes"][:, :7].copy(), "gt_names": np.array(["Car"] * n),
                           "gt_boxes_mask": np.array([True] * n)})
        raw = torch.from_numpy(np.concatenate([s["points"] for s in scenes])).to(device)
        offs = torch.from_numpy(np.cumsum([0] + [s["points"].shape[0] for s in scenes]).astype(np.int32)).to(device)
        batches.append((scenes, raw, offs))
    setup_s = time.perf_counter() - t0

    def fresh(sc):
        return {k: np.array(v, copy=True) for k, v in sc.items()}

    def host(batch):
        scenes, _, _ = batch
        res = [aug.forward(fresh(sc)) for sc in scenes]
        pts = torch.from_numpy(np.concatenate([r["points"] for r in res])).to(device)
        pre = torch.from_numpy(np.concatenate([r["pre_rot_points"] for r in res])).to(device)
        offs = torch.from_numpy(np.cumsum([0] + [r["points"].shape[0] for r in res]).astype(np.int32)).to(device)
        rot = torch.tensor([r["rot_z"] for r in res], dtype=torch.float32).to(device)
        return pts, pre, offs, rot

    def dev(batch):
        scenes, raw, offs = batch
        r = dev_aug.apply(raw, offs, dev_aug.plan(scenes))
        return r["points"], r["pre_rot_points"], r["scene_offsets"], r["rot_z"]

    fns = {"host": host, "device": dev}

    def block(mode, n, start):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(n):
            fns[mode](batches[(start + i) % len(batches)])
        torch.cuda.synchronize()      # inside the host clock
        return (time.perf_counter() - t) / n * 1e6

    np.random.seed(0)
    res = {"batch_size": args.batch_size, "rows_per_batch": [int(b[1].shape[0]) for b in batches], "db_objects": args.db_objects,
           "bank_mbytes": round(bank.rows.nbytes / 2 ** 20, 1), "setup_s": round(setup_s, 1), "batches_per_block": args.batches,
           "us_per_batch": {"host": [], "device": []}}
    for m in fns:
        block(m, args.warmup, 0)
    for a in range(args.alternations):
        for m in fns:
            res["us_per_batch"][m].append(block(m, args.batches, a))
    # the kernels alone: one plan on the device, the entry point called back to back between two events
    scenes, raw, offs = batches[0]
    plan = dev_aug.plan(scenes)
    arrs = dict(zip(AugPlan.ARRAYS, dev_aug._upload([getattr(plan, k) for k in AugPlan.ARRAYS], device)))
    n, ld, B, n_obj = raw.shape[0], raw.shape[1], plan.batch, int(plan.obj_first.shape[0])
    cap = n + plan.paste_rows
    out, pre = torch.empty((cap, ld), device=device), torch.empty((cap, ld), device=device)
    new_offs = torch.empty((B + 1,), dtype=torch.int32, device=device)
    ws_bytes = lib().btc_augment_ws_bytes(n, B, n_obj)
    ws = workspace(ws_bytes, device)
    bank_t = bank.tensor(device)

    def kernels(calls):
        for _ in range(calls):
            rc = lib().btc_augment_batch(ptr(raw), n, ld, ptr(offs), B, ptr(arrs["rm_boxes"]), ptr(arrs["rm_offsets"]), ptr(bank_t), bank_t.shape[0],
                                         ptr(arrs["obj_first"]), ptr(arrs["obj_rows"]), ptr(arrs["obj_shift"]), ptr(arrs["obj_offsets"]), n_obj,
                                         plan.paste_rows, ptr(arrs["ops"]), ptr(arrs["op_offsets"]), cap, ptr(out), ptr(pre), ptr(new_offs), ptr(ws),
                                         ws_bytes, stream_ptr())
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
    res["pasted_rows_in_that_plan"], res["removal_boxes_in_that_plan"] = plan.paste_rows, int(plan.rm_boxes.shape[0])
    res["us_per_batch_median"] = {m: statistics.median(v) for m, v in res["us_per_batch"].items()}
    res["us_per_batch_spread"] = {m: max(v) - min(v) for m, v in res["us_per_batch"].items()}
    res["kernels_us_per_batch_median"] = statistics.median(res["kernels_us_per_batch"])
    med, spr = res["us_per_batch_median"], res["us_per_batch_spread"]
    res["scenes_per_s"] = {m: args.batch_size / med[m] * 1e6 for m in med}
    res["device_below_host_by_more_than_host_spread"] = bool(med["host"] - med["device"] > spr["host"])
    return res


def main(argv=None):
    args = parse_args(argv)
    import torch
    import infer_bench
    assert torch.cuda.is_available(), "tools/augment_bench.py needs a GPU"
    with tempfile.TemporaryDirectory() as d:
        out = {"head": infer_bench.head_commit(), "alternations": args.alternations, "augment": measure(args, torch.device("cuda:0"), d)}
    print(json.dumps(out["augment"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
