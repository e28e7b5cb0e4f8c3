#!/usr/bin/env python3
"""Occupancy metrics of an eval batch: the unfused torch formulation against the fused call, alternating in ONE process.

KITTI-Car shape, batches of bench.build_batches, BtcHotPath(heads="full") in eval mode under no_grad -- the protocol of
tools/infer_bench.py --post both.  The inputs are the recorded outputs of real eval forwards (the masks of OccTargets, the occupancy
head's probability, PassOccVox's points).

  (a) alone: host clock around --calls calls ending in a device synchronisation, `unfused` and `fused` alternating --alternations times;
  (b) end to end, behind the forward: scenes/s of forward only / + fused occ_counters / + the unfused loop.

`unfused` is THE BASELINE, not code under test: this project's own torch statement of the same computation the way the reference
arranges it -- five reductions over the grid, then per scene the box-frame coordinates of every point against every valid box as an
(N, M, 3) tensor, and per threshold and scene a nonzero, a gather, a max and one .item().  Writes profiles/occ_metrics_bench.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

KEYS = ("batch_size", "batch_pred_occ_prob", "general_cls_loss_mask", "pos_mask", "neg_mask", "pos_all_num", "occ_pnts", "added_occ_b_ind",
        "gt_boxes", "gt_boxes_num")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--features", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--batches", type=int, default=4, help="distinct scene batches, cycled")
    ap.add_argument("--alternations", type=int, default=5, help="timed blocks PER MODE (at least 5 for a result that is reported)")
    ap.add_argument("--calls", type=int, default=1000, help="calls per timed block of (a) (at least 1000 for a result that is reported)")
    ap.add_argument("--forwards", type=int, default=100, help="forwards per timed block of (b) (at least 100 for a result that is reported)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occ_metrics_bench.json"))
    return ap.parse_args(argv)


def unfused_occ_metrics(bd):
    """-> the 16 counters as a list of host integers (one read-back per threshold and scene, seven more for the grid sums)"""
    import torch
    prob, pos = bd["batch_pred_occ_prob"], bd["pos_mask"]
    hit = prob >= 0.5
    row = [int(torch.sum(bd["general_cls_loss_mask"])), int(torch.sum(pos)), int(torch.sum(bd["neg_mask"])), int(torch.sum(hit)),
           int(torch.sum(pos.bool() & hit)), int(bd["pos_all_num"])]
    num = [int(k) for k in bd["gt_boxes_num"]]
    pnts, bind, gt = bd["occ_pnts"], bd["added_occ_b_ind"], bd["gt_boxes"]
    scenes = []
    for b in range(bd["batch_size"]):
        idx = torch.eq(bind, b).nonzero()[:, 0]
        if idx.shape[0] == 0:
            continue
        p, g = pnts[idx], gt[b, :num[b]]
        d = p[:, None, :3] - g[None, :, :3]
        c, s = torch.cos(g[:, 6])[None], torch.sin(g[:, 6])[None]
        loc = torch.stack([d[..., 0] * c + d[..., 1] * s, d[..., 1] * c - d[..., 0] * s, d[..., 2]], -1)
        scenes.append((p, (loc.abs() <= g[None, :, 3:6] * 0.5).all(-1).to(torch.int8)))
    covered = []
    for i in range(1, 10):
        total = 0
        for p, mask in scenes:
            sel = torch.nonzero(p[:, 3] >= i * 0.1)
            if sel.shape[0] > 0 and mask.shape[1] > 0:
                total += torch.sum(torch.max(mask[sel[:, 0], :], dim=0)[0]).item()
        covered.append(int(total))
    return row + [sum(num)] + covered


def measure(args, device):
    import torch
    import infer_bench
    from btcdet_amd import occ_metrics as om
    args.heads = "full"
    model, batches = infer_bench.build(args, "full", device)
    recorded = []
    with torch.no_grad():
        for b in batches:
            _, _, bd = model(model.prepare(b, is_train=False))
            recorded.append({k: (bd[k].clone() if torch.is_tensor(bd[k]) else bd[k]) for k in KEYS})
    fns = {"unfused": unfused_occ_metrics, "fused": om.occ_counters}
    modes = ["unfused", "fused"]
    first_unfused, first_fused = unfused_occ_metrics(recorded[0]), om.occ_counters(recorded[0]).cpu().tolist()
    res = {"batch_size": args.batch_size, "cells": int(recorded[0]["batch_pred_occ_prob"].numel()),
           "points_per_batch": [int(r["occ_pnts"].shape[0]) for r in recorded], "boxes_per_batch": [[int(k) for k in r["gt_boxes_num"]] for r in recorded],
           "counters_first_batch": first_fused, "unfused_counters_first_batch": first_unfused,
           # (exact for the grid counters; a point within float32 rounding of a face may fall on either side in the two formulations)
           "grid_counters_agree_on_first_batch": first_unfused[:7] == first_fused[:7], "box_counters_agree_on_first_batch": first_unfused[7:] == first_fused[7:],
           "calls_per_block": args.calls, "forwards_per_block": args.forwards, "alone_us_per_call": {m: [] for m in modes},
           "end_to_end_scenes_per_s": {m: [] for m in ["forward"] + modes}}

    def alone(mode, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            fns[mode](recorded[i % len(recorded)])
        torch.cuda.synchronize()      # inside the host clock
        return (time.perf_counter() - t0) / n * 1e6

    def end_to_end(mode, n, start):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for i in range(n):
                _, _, bd = model(model.prepare(batches[(start + i) % len(batches)], is_train=False))
                if mode != "forward":
                    fns[mode](bd)
        torch.cuda.synchronize()
        return n * args.batch_size / (time.perf_counter() - t0)

    for m in modes:
        alone(m, max(args.warmup, 10))
    for a in range(args.alternations):
        for m in modes:
            res["alone_us_per_call"][m].append(alone(m, args.calls))
    for m in ["forward"] + modes:
        end_to_end(m, args.warmup, 0)
    for a in range(args.alternations):
        for m in ["forward"] + modes:
            res["end_to_end_scenes_per_s"][m].append(end_to_end(m, args.forwards, a))
    for group in ("alone_us_per_call", "end_to_end_scenes_per_s"):
        res[group + "_median"] = {m: statistics.median(v) for m, v in res[group].items() if v}
        res[group + "_spread"] = {m: max(v) - min(v) for m, v in res[group].items() if v}
    med, spr = res["alone_us_per_call_median"], res["alone_us_per_call_spread"]
    res["fused_below_unfused_by_more_than_unfused_spread"] = bool(med["unfused"] - med["fused"] > spr["unfused"])
    return res


def main(argv=None):
    args = parse_args(argv)
    import torch
    import infer_bench
    assert torch.cuda.is_available(), "tools/occ_metrics_bench.py needs a GPU"
    out = {"head": infer_bench.head_commit(), "alternations": args.alternations, "occ_metrics": measure(args, torch.device("cuda:0"))}
    print(json.dumps(out["occ_metrics"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
