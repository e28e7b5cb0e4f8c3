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
    ap.add_argument("--post", choices=["none", "composed", "fused", "both"], default="none",
                    help="measure post-processing instead (heads=full): the reference's per-scene loop composed of this library's operators, "
                         "the fused detect(), or both alternating; writes --post-out")
    ap.add_argument("--post-calls", type=int, default=1000, help="post-processing calls per timed block (at least 1000 for a result that is reported)")
    ap.add_argument("--score-thresh", type=float, default=None,
                    help="SCORE_THRESH of the post-processing runs; default: the median recorded score (an untrained head scores near 0.5, the "
                         "yaml's 0.6 would leave the NMS nothing to do)")
    ap.add_argument("--post-out", default=os.path.join(ROOT, "profiles", "infer_post_bench.json"))
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


# ------------------------------------------------------------------------------------------------------------ --post
def composed_post_processing(batch_dict, post_cfg, num_class):
    """THE BASELINE, not code under test: the reference's per-scene loop (detector3d_template.py:363-476, :548-591) written over the
    operators this library had before the fused kernels -- dense_head.class_agnostic_nms (nonzero / topk / an NMS with a read-back of its
    count), iou3d_nms.boxes_iou3d_gpu, one .item() per recall threshold"""
    import torch
    from btcdet_amd import iou3d_nms
    from btcdet_amd.dense_head import class_agnostic_nms
    recall_dict, pred_dicts = {}, []
    thresh_list = post_cfg.RECALL_THRESH_LIST
    for index in range(batch_dict["batch_size"]):
        box_preds = batch_dict["batch_box_preds"][index]
        src_box_preds = box_preds
        cls_preds = batch_dict["batch_cls_preds"][index]
        src_cls_preds = cls_preds
        if not batch_dict["cls_preds_normalized"]:
            cls_preds = torch.sigmoid(cls_preds)
        cls_preds, label_preds = torch.max(cls_preds, dim=-1)
        if batch_dict.get("has_class_labels", False):
            label_preds = batch_dict["roi_labels" if "roi_labels" in batch_dict else "batch_pred_labels"][index]
        else:
            label_preds = label_preds + 1
        selected, selected_scores = class_agnostic_nms(cls_preds, box_preds, post_cfg.NMS_CONFIG, post_cfg.SCORE_THRESH)
        if post_cfg.OUTPUT_RAW_SCORE:
            selected_scores = torch.max(src_cls_preds, dim=-1)[0][selected]
        final_boxes = box_preds[selected]
        # generate_recall_record
        measured = final_boxes if "rois" not in batch_dict else src_box_preds
        rois = batch_dict["rois"][index] if "rois" in batch_dict else None
        cur_gt = batch_dict["gt_boxes"][index]
        if not recall_dict:
            recall_dict = {"gt": 0}
            for t in thresh_list:
                recall_dict["roi_%s" % t] = 0
                recall_dict["rcnn_%s" % t] = 0
        k = len(cur_gt) - 1
        while k > 0 and cur_gt[k].sum() == 0:      # (a read-back per trailing row, as in the reference)
            k -= 1
        cur_gt = cur_gt[:k + 1]
        iou3d_rcnn = None
        if cur_gt.shape[0] > 0:
            iou3d_rcnn = iou3d_nms.boxes_iou3d_gpu(measured[:, 0:7], cur_gt[:, 0:7]) if measured.shape[0] > 0 else torch.zeros((0, cur_gt.shape[0]))
            if rois is not None:
                iou3d_roi = iou3d_nms.boxes_iou3d_gpu(rois[:, 0:7], cur_gt[:, 0:7])
            for t in thresh_list:
                if iou3d_rcnn.shape[0] > 0:
                    recall_dict["rcnn_%s" % t] += (iou3d_rcnn.max(dim=0)[0] > t).sum().item()
                if rois is not None:
                    recall_dict["roi_%s" % t] += (iou3d_roi.max(dim=0)[0] > t).sum().item()
            recall_dict["gt"] += cur_gt.shape[0]
        iou3d = None if iou3d_rcnn is None or len(iou3d_rcnn) == 0 else torch.max(iou3d_rcnn, dim=1)[0]
        pred_dicts.append({"pred_boxes": final_boxes, "pred_scores": selected_scores, "pred_labels": label_preds[selected],
                           "iou": iou3d.cpu().numpy() if iou3d is not None and len(iou3d) == len(final_boxes) else None})
    return pred_dicts, recall_dict


def measure_post(args, device):
    """(a) post-processing alone on the recorded head outputs of real eval forwards, host clock around --post-calls calls ending in a device
    synchronise, composed and fused alternating; (b) end-to-end scenes/s: forward only / + fused detect / + composed loop"""
    import copy
    import torch
    from btcdet_amd import post_processing as pp
    model, batches = build(args, "full", device)
    post_cfg = copy.deepcopy(model.cfg.MODEL.POST_PROCESSING)
    num_class = len(model.cfg.CLASS_NAMES)
    keys = ("batch_size", "batch_cls_preds", "batch_box_preds", "cls_preds_normalized", "rois", "roi_labels", "has_class_labels", "gt_boxes")
    recorded = []
    with torch.no_grad():
        for b in batches:
            _, _, bd = model(model.prepare(b, is_train=False))
            recorded.append({k: (bd[k].clone() if torch.is_tensor(bd[k]) else bd[k]) for k in keys if k in bd})
    scores = torch.cat([torch.sigmoid(r["batch_cls_preds"]).max(-1)[0].reshape(-1) for r in recorded])
    if args.score_thresh is None:
        args.score_thresh = float(scores.median())
    post_cfg["SCORE_THRESH"] = args.score_thresh
    modes = ["composed", "fused"] if args.post == "both" else [args.post]
    fns = {"composed": lambda bd: composed_post_processing(bd, post_cfg, num_class), "fused": lambda bd: pp.detect(bd, post_cfg, num_class)}
    want, _ = composed_post_processing(recorded[0], post_cfg, num_class)
    got, _ = pp.post_processing(recorded[0], post_cfg, num_class)
    res = {"batch_size": args.batch_size, "boxes_per_scene": int(recorded[0]["batch_box_preds"].shape[1]), "score_thresh": args.score_thresh,
           "detections_first_batch": [int(len(p["pred_scores"])) for p in got],
           "composed_and_fused_agree_on_first_batch": all(torch.equal(a["pred_boxes"], b["pred_boxes"]) for a, b in zip(want, got)),
           "calls_per_block": args.post_calls, "alone_us_per_call": {m: [] for m in modes}, "end_to_end_scenes_per_s": {m: [] for m in ["forward"] + modes}}

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
            res["alone_us_per_call"][m].append(alone(m, args.post_calls))
    for m in ["forward"] + modes:
        end_to_end(m, args.warmup, 0)
    for a in range(args.alternations):
        for m in ["forward"] + modes:
            res["end_to_end_scenes_per_s"][m].append(end_to_end(m, args.forwards, a))
    for group in ("alone_us_per_call", "end_to_end_scenes_per_s"):
        res[group + "_median"] = {m: statistics.median(v) for m, v in res[group].items() if v}
        res[group + "_spread"] = {m: max(v) - min(v) for m, v in res[group].items() if v}
    if args.post == "both":
        med, spr = res["alone_us_per_call_median"], res["alone_us_per_call_spread"]
        res["fused_below_composed_by_more_than_composed_spread"] = bool(med["composed"] - med["fused"] > spr["composed"])
    return res


def main(argv=None):
    args = parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "tools/infer_bench.py needs a GPU"
    device = torch.device("cuda:0")
    if args.post != "none":
        out = {"head": head_commit(), "alternations": args.alternations, "post": measure_post(args, device)}
        print(json.dumps(out["post"]), flush=True)
        os.makedirs(os.path.dirname(args.post_out), exist_ok=True)
        with open(args.post_out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return out
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
