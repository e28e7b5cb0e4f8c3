#!/usr/bin/env python3
"""Anchor-head loss: the torch formulation of get_loss() against the fused calls, alternating in ONE process.

KITTI-Car head shape (200 x 176 locations, two rotations: 70 400 anchors), batch size 2, boxes of synth.make_scene, targets from
DeviceTargetAssigner.  Two AnchorHeadSingle of the same configuration, one without LOSS_CONFIG.DEVICE (`torch`: THE BASELINE -- the
reference's formulation in dense_head.get_loss, the code of the parent commit) and one with it (`fused`: btcdet_amd/anchor_loss.py).

What is timed: get_loss() plus backward() to the three prediction tensors (leaves; their .grad is dropped between calls).
Host clock around --calls calls ending in a device synchronisation, `torch` and `fused` alternating --alternations times; per route the
median block, and the spread (max - min) of the blocks.  Kernel launches per call are counted as tools/anchor_targets_bench.py counts
them.  Not measured here: the effect on a --heads full training step (the step has its own bench).
Writes profiles/anchor_loss_bench.json.
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


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--batches", type=int, default=4, help="distinct box batches, cycled")
    ap.add_argument("--alternations", type=int, default=5, help="timed blocks PER ROUTE (at least 5 for a result that is reported)")
    ap.add_argument("--calls", type=int, default=500, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_loss_bench.json"))
    return ap.parse_args(argv)


def measure(args, device):
    import numpy as np
    import torch
    from anchor_targets_bench import head_cfg, launches
    from btcdet_amd import synth
    from btcdet_amd.dense_head import AnchorHeadSingle
    B = args.batch_size
    heads = {}
    for route in ("torch", "fused"):
        cfg = head_cfg(True)                            # targets from DeviceTargetAssigner on both routes
        if route == "fused":
            cfg.LOSS_CONFIG["DEVICE"] = True
        heads[route] = AnchorHeadSingle(cfg, input_channels=8, num_class=1, class_names=["Car"], grid_size=np.array([1408, 1600, 40]),
                                        point_cloud_range=np.array([0, -40, -3, 70.4, 40, 1], dtype=np.float32)).to(device)
    assert heads["fused"].device_loss and not heads["torch"].device_loss
    anchors = heads["torch"].anchors(device)
    targets = []
    for k in range(args.batches):
        boxes = [synth.make_scene(41 + B * k + s, az_step=2.0)["gt_boxes"] for s in range(B)]
        gt = np.zeros((B, max(len(b) for b in boxes) + 1, 8), np.float32)
        for i, b in enumerate(boxes):
            gt[i, :len(b)] = b
        targets.append(heads["torch"].target_assigner.assign_targets(anchors, torch.from_numpy(gt).to(device)))
    torch.manual_seed(0)
    preds = dict(cls_preds=(torch.randn(B, 200, 176, 2, device=device) - 4.0).requires_grad_(True),
                 box_preds=(torch.randn(B, 200, 176, 14, device=device) * 0.3).requires_grad_(True),
                 dir_cls_preds=torch.randn(B, 200, 176, 4, device=device).requires_grad_(True))

    def fn(route):
        h = heads[route]

        def call(i=0):
            t = targets[i % len(targets)]
            h.forward_ret_dict = dict(preds, box_cls_labels=t["box_cls_labels"].clone() if route == "torch" else t["box_cls_labels"],
                                      box_reg_targets=t["box_reg_targets"])
            for p in preds.values():
                p.grad = None
            loss, tb = h.get_loss()
            loss.backward()
            return loss, tb
        return call

    routes = ["torch", "fused"]
    (la, ta), ga = fn("torch")(), {k: p.grad.clone() for k, p in preds.items()}
    (lb, tb), gb = fn("fused")(), {k: p.grad.clone() for k, p in preds.items()}
    res = {"batch_size": B, "anchors": int(targets[0]["box_cls_labels"].shape[1]),
           "positives_per_batch": [[int(n) for n in (t["box_cls_labels"] > 0).sum(1)] for t in targets], "calls_per_block": args.calls,
           "loss": {"torch": float(la), "fused": float(lb)}, "tb_keys_agree": list(ta) == list(tb),
           "grad_max_abs_diff": {k: float((ga[k] - gb[k]).abs().max()) for k in preds},
           "launches_per_call": {r: launches(fn(r)) for r in routes}, "us_per_call": {r: [] for r in routes},
           "note": "the torch route's block includes one clone of the labels per call: its get_loss overwrites them in place"}

    def block(route, n):
        f = fn(route)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            f(i)
        torch.cuda.synchronize()      # inside the host clock
        return (time.perf_counter() - t0) / n * 1e6

    for r in routes:
        block(r, max(args.warmup, 10))
    for _ in range(args.alternations):
        for r in routes:
            res["us_per_call"][r].append(block(r, args.calls))
    res["us_per_call_median"] = {r: statistics.median(v) for r, v in res["us_per_call"].items()}
    res["us_per_call_spread"] = {r: max(v) - min(v) for r, v in res["us_per_call"].items()}
    med, spr = res["us_per_call_median"], res["us_per_call_spread"]
    res["fused_below_torch_by_more_than_torch_spread"] = bool(med["torch"] - med["fused"] > spr["torch"])
    return res


def main(argv=None):
    args = parse_args(argv)
    import torch
    import infer_bench
    assert torch.cuda.is_available(), "tools/anchor_loss_bench.py needs a GPU"
    out = {"head": infer_bench.head_commit(), "alternations": args.alternations, "anchor_loss": measure(args, torch.device("cuda:0"))}
    print(json.dumps(out["anchor_loss"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
