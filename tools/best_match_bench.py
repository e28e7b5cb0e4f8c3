#!/usr/bin/env python3
"""`bm_points` of a batch: the host route of the add_multi_best_match step against the resident TemplateBank, alternating in ONE process.

KITTI-Car shape, batch size 2, the scans and the synthetic ground-truth database of tools/augment_bench.py, the model config's queue
with the step where the shipped configuration has it: gt_sampling -> add_multi_best_match -> random_world_flip ->
random_world_scaling -> random_world_rotation with SAVE_PRE_ROT.  The templates are SYNTHETIC: one pickle per database object and per
scene box, --template-rows-min .. --template-rows-max rows each (uniform).  How many rows a real KITTI template has, and so how large a real
bank is, has not been measured anywhere: the row counts used are written into the result.

  host   DeviceAugmentor(augmentor, bank).plan + apply: plan() opens one pickle per box, runs one np.einsum per box and concatenates;
         apply() uploads the set and runs btc_world_transform over it;
  bank   DeviceAugmentor(augmentor, bank, templates).plan + apply: plan() records one placement per box, apply() runs
         btc_place_templates from the resident bank;
  launch btc_place_templates alone with a plan that is already on the device, between two device events.

`host` is THE BASELINE, not code under test.  Both routes do everything else the same (the sampler, the scan's kernels, the read-back of
apply), so the difference of the two is the step's.  Host clock around --batches batches ending in a device synchronisation, `host` and
`bank` alternating --alternations times.  Writes profiles/best_match_bench.json.
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
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import augment_bench  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--scene-batches", type=int, default=4, help="distinct scene batches, cycled")
    ap.add_argument("--db-objects", type=int, default=14357, help="objects of the synthetic database (KITTI train split: 14 357 cars)")
    ap.add_argument("--template-rows-min", type=int, default=200)
    ap.add_argument("--template-rows-max", type=int, default=1000)
    ap.add_argument("--alternations", type=int, default=5, help="timed blocks PER ROUTE (at least 5 for a result that is reported)")
    ap.add_argument("--batches", type=int, default=50, help="batches per timed block (at least 50 for a result that is reported)")
    ap.add_argument("--kernel-calls", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_match_bench.json"))
    return ap.parse_args(argv)


def queue():
    q = augment_bench.queue()
    q["AUG_CONFIG_LIST"].insert(1, augment_bench.Cfg(NAME="add_multi_best_match", LOAD_POINT_FEATURES=3))
    return q


def measure(args, device, db_root):
    import numpy as np
    import torch
    from btcdet_amd import synth
    from btcdet_amd._lib import lib, ptr, stream_ptr
    from btcdet_amd.device_augmentor import AugPlan, DataAugmentor, DeviceAugmentor, ObjectBank, TemplateBank
    t0 = time.perf_counter()
    infos = augment_bench.make_database(db_root, args.db_objects)
    bank = ObjectBank(db_root, infos, 4)
    bank.tensor(device)
    batches, keys = [], [(int(e["image_idx"]), int(e["gt_idx"])) for e in infos["Car"]]
    for k in range(args.scene_batches):
        scenes = []
        for b in range(args.batch_size):
            s = synth.make_scene(7000 + 10 * k + b)
            n = s["gt_boxes"].shape[0]
            frame = 900000 + 10 * k + b                     # (past every image_idx of the database)
            scenes.append({"points": s["points"], "gt_boxes": s["gt_boxes"][:, :7].copy(), "gt_names": np.array(["Car"] * n),
                           "gt_boxes_mask": np.array([True] * n), "frame_id": "%06d" % frame})
            keys += [(frame, i) for i in range(n)]
        raw = torch.from_numpy(np.concatenate([s["points"] for s in scenes])).to(device)
        offs = torch.from_numpy(np.cumsum([0] + [s["points"].shape[0] for s in scenes]).astype(np.int32)).to(device)
        batches.append((scenes, raw, offs))
    rng = np.random.default_rng(11)
    troot = os.path.join(db_root, "bm_car")
    os.makedirs(troot)
    for img, gt in keys:
        rows = int(rng.integers(args.template_rows_min, args.template_rows_max + 1))
        with open(os.path.join(troot, "{}_{}.pkl".format(img, gt)), "wb") as f:
            pickle.dump(rng.uniform(-2, 2, rows * 3).astype(np.float32), f)
    import pathlib
    roots = {"Car": pathlib.Path(troot)}
    t1 = time.perf_counter()
    templates = TemplateBank(roots)
    templates.tensor(device)
    torch.cuda.synchronize()
    bank_load_s = time.perf_counter() - t1
    def augmentor():      # (one per route: each sampler walks its own permutation of the database)
        return DataAugmentor(db_root, queue(), ["Car"], db_infos=infos, template_root=roots)
    routes = {"host": DeviceAugmentor(augmentor(), bank), "bank": DeviceAugmentor(augmentor(), bank, templates)}
    setup_s = time.perf_counter() - t0

    def run(mode, batch):
        scenes, raw, offs = batch
        d = routes[mode]
        return d.apply(raw, offs, d.plan(scenes))

    def block(mode, n, start):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(n):
            run(mode, batches[(start + i) % len(batches)])
        torch.cuda.synchronize()      # inside the host clock
        return (time.perf_counter() - t) / n * 1e6

    np.random.seed(0)
    res = {"batch_size": args.batch_size, "rows_per_batch": [int(b[1].shape[0]) for b in batches], "db_objects": args.db_objects,
           "templates": len(templates.table), "template_rows": "uniform %d..%d (synthetic; real KITTI templates unmeasured)" %
           (args.template_rows_min, args.template_rows_max), "template_bank_mbytes": round(templates.nbytes / 2 ** 20, 1),
           "template_bank_load_s": round(bank_load_s, 1), "setup_s": round(setup_s, 1), "batches_per_block": args.batches,
           "us_per_batch": {"host": [], "bank": []}}
    # both routes give the same bytes from the same draws (fresh samplers, same seed), before anything is timed
    a = run("host", batches[0])["special"]["bm_points"]
    np.random.seed(0)
    b = run("bank", batches[0])["special"]["bm_points"]
    assert a[1].tolist() == b[1].tolist() and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), "the two routes differ"
    for m in routes:
        block(m, args.warmup, 0)
    for alt in range(args.alternations):
        for m in routes:
            res["us_per_batch"][m].append(block(m, args.batches, alt))
    # the launch alone: one plan on the device, the entry point called back to back between two events
    scenes, raw, offs = batches[0]
    d = routes["bank"]
    plan = d.plan(scenes)
    names = AugPlan.ARRAYS + AugPlan.BM_ARRAYS
    arrs = dict(zip(names, d._upload([getattr(plan, k) for k in names], device)))
    tb = templates.tensor(device)
    n_pl, n_out = int(plan.bm_first.shape[0]), plan.bm_rows_total
    res["launch_us"] = {}
    for out_ld in (3, 4):
        out = torch.empty((n_out, out_ld), device=device)

        def launches(calls):
            for _ in range(calls):
                rc = lib().btc_place_templates(ptr(tb), tb.shape[0], ptr(arrs["bm_first"]), ptr(arrs["bm_rows"]), ptr(arrs["bm_place"]),
                                               ptr(arrs["bm_offsets"]), ptr(arrs["bm_row_offsets"]), n_pl, plan.batch, ptr(arrs["ops"]),
                                               ptr(arrs["op_offsets"]), n_out, out_ld, ptr(out), stream_ptr())
                assert rc == 0
        launches(20)
        ts = []
        for _ in range(args.alternations):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            launches(args.kernel_calls)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / args.kernel_calls)
        res["launch_us"]["out_ld_%d" % out_ld] = ts
    res["placements_in_that_plan"], res["bm_rows_in_that_plan"] = n_pl, n_out
    res["us_per_batch_median"] = {m: statistics.median(v) for m, v in res["us_per_batch"].items()}
    res["us_per_batch_spread"] = {m: max(v) - min(v) for m, v in res["us_per_batch"].items()}
    res["launch_us_median"] = {k: statistics.median(v) for k, v in res["launch_us"].items()}
    med, spr = res["us_per_batch_median"], res["us_per_batch_spread"]
    res["bank_below_host_by_more_than_host_spread"] = bool(med["host"] - med["bank"] > spr["host"])
    return res


def main(argv=None):
    args = parse_args(argv)
    import torch
    import infer_bench
    assert torch.cuda.is_available(), "tools/best_match_bench.py needs a GPU"
    with tempfile.TemporaryDirectory() as d:
        out = {"head": infer_bench.head_commit(), "alternations": args.alternations, "best_match": measure(args, torch.device("cuda:0"), d)}
    print(json.dumps(out["best_match"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
