#!/usr/bin/env python3
"""Inference throughput with the eval-mode conv + BatchNorm fold on and off (tuning key 23), alternating in ONE process.

KITTI-Car shape, batches of bench.build_batches, BtcHotPath in eval mode under no_grad: heads none (to the BEV map) and heads="full"
(to batch_cls_preds / batch_box_preds).  After a warm-up of both settings the fold is switched --alternations times; every alternation
times --forwards forwards with the device synchronised inside the host clock.  The folded layers per forward are COUNTED (the compiled
binding's eval_fold_calls), not assumed.  Writes profiles/infer_bench.json.

Kernel launches per forward come from a separate trace of the same tool:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/infer_bench.py --fold 0 --forwards N --alternations 1 --heads none
and the same with --fold 1 (a fixed setting instead of alternating); launches(fold) = launches(no fold) - 2 x folded layers.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EVAL_FOLD = 23


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--heads", choices=["none", "full", "both"], default="both")
    ap.add_argument("--features", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--batches", type=int, default=4, help="distinct scene batches, cycled")
    ap.add_argument("--alternations", type=int, default=5, help="timed blocks PER SETTING of the fold (at least 5 for a result that is reported)")
    ap.add_argument("--forwards", type=int, default=100, help="forwards per timed block (at least 100 for a result that is reported)")
    ap.add_argument("--warmup", type=int, default=10, help="forwards per setting before the first timed block")
    ap.add_argument("--fold", type=int, choices=[0, 1], default=None, help="tracing runs: keep key 23 at this value instead of alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer_bench.json"))
    return ap.parse_args(argv)


def head_commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None


def build(args, heads, device):
    import numpy as np
    import torch
    import bench
    from btcdet_amd.btc_path import BtcHotPath
    from btcdet_amd.config import load_cfg
    cfg = load_cfg()
    if args.features == "bf16":
        cfg.MODEL.OCC.BACKBONE_3D["FEATURE_DTYPE"] = "bf16"
        cfg.MODEL.BACKBONE_3D["FEATURE_DTYPE"] = "bf16"
    torch.manual_seed(0)
    np.random.seed(0)
    model = BtcHotPath(cfg, device=device, heads=None if heads == "none" else heads).to(device)
    batches = bench.build_batches(args.batches, 0, device, batch_size=args.batch_size)
    model.train()
    with torch.no_grad():      # running statistics other than their initial values
        for b in batches[:2]:
            model(model.prepare(b))
    model.eval()
    return model, batches


def run_block(model, batches, n, start=0):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for i in range(n):
            model(model.prepare(batches[(start + i) % len(batches)], is_train=False))
    torch.cuda.synchronize()      # inside the host clock
    return time.perf_counter() - t0


def measure(args, heads, device):
    from btcdet_amd import _lib
    L, F = _lib.lib(), _lib.fast()
    assert F is not None, "the compiled binding is not built"
    model, batches = build(args, heads, device)
    settings = [args.fold] if args.fold is not None else [1, 0]      # key values: 1 = unfolded first, then folded, alternating
    res = {"heads": heads, "features": args.features, "batch_size": args.batch_size, "forwards_per_block": args.forwards,
           "unfolded_scenes_per_s": [], "folded_scenes_per_s": []}
    try:
        for key in settings:
            L.btc_tune_set(EVAL_FOLD, key)
            run_block(model, batches, args.warmup)
        for key in settings:       # folded layers of one forward, counted
            L.btc_tune_set(EVAL_FOLD, key)
            c0 = F.eval_fold_calls()
            run_block(model, batches, 1)
            res["folded_layers_per_forward" if key == 0 else "folded_layers_per_forward_with_key_1"] = F.eval_fold_calls() - c0
        for a in range(args.alternations):
            for key in settings:
                L.btc_tune_set(EVAL_FOLD, key)
                dt = run_block(model, batches, args.forwards, start=a)
                res["folded_scenes_per_s" if key == 0 else "unfolded_scenes_per_s"].append(args.forwards * args.batch_size / dt)
    finally:
        L.btc_tune_set(EVAL_FOLD, 0)
    for k in ("unfolded", "folded"):
        v = res[k + "_scenes_per_s"]
        if v:
            res[k + "_median"] = statistics.median(v)
            res[k + "_spread"] = max(v) - min(v)
    return res


def main(argv=None):
    args = parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "tools/infer_bench.py needs a GPU"
    device = torch.device("cuda:0")
    out = {"head": head_commit(), "alternations": args.alternations, "runs": []}
    for heads in (["none", "full"] if args.heads == "both" else [args.heads]):
        out["runs"].append(measure(args, heads, device))
        print(json.dumps(out["runs"][-1]), flush=True)
    if args.fold is None:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return out


if __name__ == "__main__":
    main()
