#!/usr/bin/env python3
"""Anchor-head targets and boxes: the torch formulation against the fused calls, alternating in ONE process.

KITTI-Car head shape (200 x 176 locations, two rotations: 70 400 anchors), batch size 2, boxes of synth.make_scene.  Two AnchorHeadSingle
of the same configuration, one without TARGET_ASSIGNER_CONFIG.DEVICE (`torch`: THE BASELINE -- dense_head.AxisAlignedTargetAssigner and
ResidualCoder.decode_torch, the code of the parent commit) and one with it (`fused`: btcdet_amd/anchor_targets.py).

  assign   target_assigner.assign_targets alone
  decode   generate_predicted_boxes alone (random regression output and direction logits)
  both     one after the other
Host clock around --calls calls ending in a device synchronisation, `torch` and `fused` alternating --alternations times; per route the
median block, and the spread (max - min) of the blocks.  Kernel launches per call are counted with torch.profiler where it reports
device activity.  Not measured here: the two calls behind a --heads full training step (the step has its own bench).
Writes profiles/anchor_targets_bench.json.
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


class ED(dict):
    __getattr__ = dict.get
    __setattr__ = dict.__setitem__

    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in dict(d or {}, **kw).items():
            self[k] = ED(v) if isinstance(v, dict) else ([ED(x) if isinstance(x, dict) else x for x in v] if isinstance(v, list) else v)


def head_cfg(device):
    tgt = dict(NAME="AxisAlignedTargetAssigner", POS_FRACTION=-1.0, SAMPLE_SIZE=512, NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False, BOX_CODER="ResidualCoder")
    if device:
        tgt["DEVICE"] = True
    return ED(CLASS_AGNOSTIC=False, USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
              ANCHOR_GENERATOR_CONFIG=[dict(class_name="Car", anchor_sizes=[[3.9, 1.6, 1.56]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-1.78],
                                            align_center=False, feature_map_stride=8, matched_threshold=0.6, unmatched_threshold=0.45)],
              TARGET_ASSIGNER_CONFIG=tgt, LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, code_weights=[1.0] * 7)))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--batches", type=int, default=4, help="distinct box batches, cycled")
    ap.add_argument("--alternations", type=int, default=5, help="timed blocks PER ROUTE (at least 5 for a result that is reported)")
    ap.add_argument("--calls", type=int, default=2000, help="calls per timed block (at least 2000 for a result that is reported: a block of the fused route is then 40 ms)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_targets_bench.json"))
    return ap.parse_args(argv)


def launches(fn):
    """device kernels one call of fn enqueues, or None where the profiler reports no device activity"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception as e:      # a profiler that cannot start must not cost the timings
        print("launch count unavailable: %r" % (e,), flush=True)
        return None


def measure(args, device):
    import numpy as np
    import torch
    from btcdet_amd import synth
    from btcdet_amd.dense_head import AnchorHeadSingle
    B = args.batch_size
    heads = {}
    for route in ("torch", "fused"):
        heads[route] = AnchorHeadSingle(head_cfg(route == "fused"), input_channels=8, num_class=1, class_names=["Car"], grid_size=np.array([1408, 1600, 40]),
                                        point_cloud_range=np.array([0, -40, -3, 70.4, 40, 1], dtype=np.float32)).to(device)
    gts = []
    for k in range(args.batches):
        boxes = [synth.make_scene(41 + B * k + s, az_step=2.0)["gt_boxes"] for s in range(B)]
        gt = np.zeros((B, max(len(b) for b in boxes) + 1, 8), np.float32)
        for i, b in enumerate(boxes):
            gt[i, :len(b)] = b
        gts.append(torch.from_numpy(gt).to(device))
    torch.manual_seed(0)
    cls = torch.randn(B, 200, 176, 2, device=device)
    box = torch.randn(B, 200, 176, 14, device=device) * 0.3
    dirs = torch.randn(B, 200, 176, 4, device=device)
    anchors = heads["torch"].anchors(device)

    def fn(route, what):
        h = heads[route]

        def assign(i=0):
            return h.target_assigner.assign_targets(anchors, gts[i % len(gts)])

        def decode(i=0):
            return h.generate_predicted_boxes(B, cls, box, dirs)

        def both(i=0):
            assign(i)
            return decode(i)
        return {"assign": assign, "decode": decode, "both": both}[what]

    routes, whats = ["torch", "fused"], ["assign", "decode", "both"]
    a, b = fn("torch", "assign")(), fn("fused", "assign")()
    ta, tb = fn("torch", "decode")()[1], fn("fused", "decode")()[1]
    res = {"batch_size": B, "anchors": int(a["box_cls_labels"].shape[1]), "boxes_per_batch": [[int((g[i].abs().sum(-1) > 0).sum()) for i in range(B)] for g in gts],
           "calls_per_block": args.calls,
           "labels_agree_on_first_batch": bool(torch.equal(a["box_cls_labels"], b["box_cls_labels"])),
           "targets_max_abs_diff_on_first_batch": float((a["box_reg_targets"] - b["box_reg_targets"]).abs().max()),
           "boxes_max_abs_diff": float((ta - tb).abs().max()),
           "launches_per_call": {w: {r: launches(fn(r, w)) for r in routes} for w in ("assign", "decode")},
           "us_per_call": {w: {r: [] for r in routes} for w in whats}}

    def block(route, what, n):
        f = fn(route, what)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            f(i)
        torch.cuda.synchronize()      # inside the host clock
        return (time.perf_counter() - t0) / n * 1e6

    for w in whats:
        for r in routes:
            block(r, w, max(args.warmup, 10))
        for _ in range(args.alternations):
            for r in routes:
                res["us_per_call"][w][r].append(block(r, w, args.calls))
    res["us_per_call_median"] = {w: {r: statistics.median(v) for r, v in d.items()} for w, d in res["us_per_call"].items()}
    res["us_per_call_spread"] = {w: {r: max(v) - min(v) for r, v in d.items()} for w, d in res["us_per_call"].items()}
    med, spr = res["us_per_call_median"], res["us_per_call_spread"]
    res["fused_below_torch_by_more_than_torch_spread"] = {w: bool(med[w]["torch"] - med[w]["fused"] > spr[w]["torch"]) for w in whats}
    return res


def main(argv=None):
    args = parse_args(argv)
    import torch
    import infer_bench
    assert torch.cuda.is_available(), "tools/anchor_targets_bench.py needs a GPU"
    out = {"head": infer_bench.head_commit(), "alternations": args.alternations, "anchor_targets": measure(args, torch.device("cuda:0"))}
    print(json.dumps(out["anchor_targets"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
