#!/usr/bin/env python3
"""ROI-head targets: the torch route against the fused call, alternating in ONE process.

KITTI-Car ROI head (ROI_PER_IMAGE 128, SAMPLE_ROI_BY_EACH_CLASS, roi_iou scores), N = the TRAIN NMS_POST_MAXSIZE of the configuration (or
--n), batch size 2, boxes of synth.make_scene, proposals in the manner of tests/golden/common.py::roi_target_inputs: a third jittered lightly
around the boxes (foreground), a third jittered more (hard background), the rest anywhere in the range (easy background).

  torch   canonical_targets(ProposalTargetLayer(...)(batch)): THE BASELINE -- btcdet_amd/roi_targets.py, the code of the parent commit
  fused   DeviceProposalTargets(...)(batch): btcdet_amd/roi_targets_device.py, one launch plus its one torch.rand
Both draw their own uniforms, as they do in training.  Host clock around --calls calls ending in a device synchronisation, `torch` and
`fused` alternating --alternations times; per route the median block, and the spread (max - min) of the blocks.  Kernel launches per call
are counted with torch.profiler where it reports device activity.  Not measured here: the call behind a --heads full training step (the
step has its own bench).  --lib times a library built with other tile constants (profiles/README.md).
Writes profiles/roi_targets_bench.json.
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

from anchor_targets_bench import launches  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--n", type=int, default=0, help="proposals per scene (0: the TRAIN NMS_POST_MAXSIZE of the configuration)")
    ap.add_argument("--batches", type=int, default=4, help="distinct batches, cycled")
    ap.add_argument("--alternations", type=int, default=5, help="timed blocks PER ROUTE (at least 5 for a result that is reported)")
    ap.add_argument("--calls", type=int, default=1000, help="calls per timed block (at least 1000 for a result that is reported)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lib", default=None, help="load this libbtcdet_hip.so instead of the package's (a build with other tile constants)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_targets_bench.json"))
    return ap.parse_args(argv)


def make_batch(B, N, seed, device):
    """rois (B, N, 7), scores, labels, gt_boxes (B, G + 1, 8) zero-padded: thirds of foreground / hard / easy proposals around synthetic boxes"""
    import numpy as np
    import torch
    from btcdet_amd import synth
    rng = np.random.default_rng(seed)
    boxes = [synth.make_scene(61 + B * seed + s)["gt_boxes"].astype(np.float32) for s in range(B)]
    gt = np.zeros((B, max(len(b) for b in boxes) + 1, 8), np.float32)
    rois = np.zeros((B, N, 7), np.float32)
    labels = np.ones((B, N), np.int64)
    k = np.arange(N)
    for i, bx in enumerate(boxes):
        gt[i, :len(bx)] = bx
        u = rng.uniform(0, 1, (N, 7)).astype(np.float32)
        r = bx[k % len(bx), :7].copy()
        labels[i] = bx[k % len(bx), 7].astype(np.int64)
        scale = np.where(k % 3 == 0, 0.15, np.where(k % 3 == 1, 1.0, 0.0)).astype(np.float32)[:, None]
        r[:, 0:3] += (u[:, 0:3] - 0.5) * np.array([2.0, 2.0, 0.5], np.float32) * scale
        r[:, 3:6] *= 1.0 + (u[:, 3:6] - 0.5) * 0.3 * scale
        r[:, 6] += (u[:, 6] - 0.5) * 0.8 * scale[:, 0]
        far = k % 3 == 2
        r[far, 0], r[far, 1], r[far, 6] = 5.0 + u[far, 0] * 60.0, (u[far, 1] - 0.5) * 70.0, (u[far, 6] - 0.5) * 6.0
        rois[i] = r
    scores = rng.uniform(0, 1, (B, N)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(device)
    return {"batch_size": B, "rois": t(rois), "roi_scores": t(scores), "roi_labels": t(labels), "gt_boxes": t(gt)}


def measure(args, device):
    import torch
    from btcdet_amd.config import load_cfg
    from btcdet_amd.roi_targets import ProposalTargetLayer, canonical_targets
    from btcdet_amd.roi_targets_device import DeviceProposalTargets
    roi_head = load_cfg().MODEL.ROI_HEAD
    cfg = roi_head.TARGET_CONFIG
    B = args.batch_size
    N = args.n or int(roi_head.NMS_CONFIG["TRAIN"]["NMS_POST_MAXSIZE"])
    batches = [make_batch(B, N, s, device) for s in range(args.batches)]
    layers = {"torch": ProposalTargetLayer(cfg), "fused": DeviceProposalTargets(cfg)}

    def fn(route):
        if route == "torch":
            return lambda i=0: canonical_targets(layers["torch"](batches[i % len(batches)]))
        return lambda i=0: layers["fused"](batches[i % len(batches)])

    routes = ["torch", "fused"]
    u = torch.rand((B, 4, max(N, int(cfg.ROI_PER_IMAGE))), device=device)
    a = canonical_targets(layers["torch"](batches[0], uniforms=u))
    b = layers["fused"](batches[0], uniforms=u)
    exact = [k for k in a if k != "gt_of_rois"]
    res = {"batch_size": B, "proposals": N, "rois_per_image": int(cfg.ROI_PER_IMAGE), "boxes_per_batch": [[int((g["gt_boxes"][i].abs().sum(-1) > 0).sum()) for i in range(B)] for g in batches],
           "calls_per_block": args.calls, "library": args.lib or "package",
           "foreground_per_scene_on_first_batch": [int(v) for v in (b["max_overlaps"] >= min(cfg.REG_FG_THRESH, cfg.CLS_FG_THRESH)).sum(1).tolist()],
           "outputs_equal_on_the_same_uniforms": bool(all(torch.equal(a[k], b[k]) for k in exact)),
           "gt_of_rois_max_abs_diff_on_the_same_uniforms": float((a["gt_of_rois"] - b["gt_of_rois"]).abs().max()),
           "launches_per_call": {r: launches(fn(r)) for r in routes}, "us_per_call": {r: [] for r in routes}}

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
    if args.lib:
        from btcdet_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
        os.environ["BTC_FASTPATH"] = "0"      # the compiled binding belongs to the package's library
    assert torch.cuda.is_available(), "tools/roi_targets_bench.py needs a GPU"
    out = {"head": infer_bench.head_commit(), "alternations": args.alternations, "roi_targets": measure(args, torch.device("cuda:0"))}
    print(json.dumps(out["roi_targets"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
