"""Shared by the post-processing golden generator and its tests: the golden CASES with their regenerable inputs, and a numpy restatement
of the reference's Detector3DTemplate.post_processing (class-agnostic branch) over the C oracle's NMS and 3-D IoU.

The restatement is pinned to the golden file (tests/golden/det_post.npz, written by the REAL reference classes) by
tests/test_det_post_cpu.py; the GPU tests then use it as the expectation for seeded cases the golden file does not hold.
Imports nothing that needs a GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(HERE, "golden"), os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import common  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "det_post.npz")

# the reference's POST_PROCESSING block (tools/cfgs/model_configs/btcdet_kitti_car.yaml:317-328)
BASE_CFG = {"RECALL_THRESH_LIST": [0.3, 0.5, 0.7], "SCORE_THRESH": 0.6, "OUTPUT_RAW_SCORE": False, "EVAL_METRIC": "kitti",
            "NMS_CONFIG": {"MULTI_CLASSES_NMS": False, "NMS_TYPE": "nms_gpu", "NMS_THRESH": 0.1, "NMS_PRE_MAXSIZE": 4096, "NMS_POST_MAXSIZE": 500}}

# name -> what differs from: n = 100 boxes per scene, one class, logits, no rois, no class labels, BASE_CFG.
# The three scenes of common.roi_target_inputs: two with ground truth, the third WITHOUT (one all-zero row counts as one ground truth).
CASES = {
    "configured": dict(rois=True, labels="roi_labels"),                 # as BtcNet runs it: rois + roi_labels + has_class_labels
    "no_rois": dict(),
    "class_labels": dict(labels="batch_pred_labels"),
    "raw_score": dict(cfg={"OUTPUT_RAW_SCORE": True}),
    "normalized": dict(normalized=True),
    "nms_normal": dict(nms={"NMS_TYPE": "nms_normal_gpu"}),
    "three_class": dict(num_class=3, rois=True),
    "truncate": dict(nms={"NMS_POST_MAXSIZE": 5}),
    "pre_max": dict(nms={"NMS_PRE_MAXSIZE": 12}),
    "no_detections": dict(quiet_scene=1, rois=True, labels="roi_labels"),   # scene 1: every logit -3
    "large": dict(n=4000),                                               # the path behind the anchor head (n > 1024)
}
# hash salts of the inputs: 400 + 10 i, moved on where the generator's margin assertions (gen_det_post_golden.py) did not hold
SALT = {name: 400 + 10 * i for i, name in enumerate(CASES)}
SALT.update(raw_score=442, three_class=487)
LARGE_SEED = 50       # seed of the n = 4000 case's permutations: the first one on which the margins hold


def case_cfg(name):
    c = CASES[name]
    cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in BASE_CFG.items()}
    cfg.update(c.get("cfg", {}))
    cfg["NMS_CONFIG"].update(c.get("nms", {}))
    return cfg


def case_inputs(name):
    """-> batch_dict of numpy arrays (+ plain values) and num_class; regenerated from integer hashes, identical on every machine"""
    c = CASES[name]
    n, C, salt = c.get("n", 100), c.get("num_class", 1), SALT[name]
    inp = common.roi_target_inputs(n_rois=n)
    B = inp["batch_size"]
    rois = inp["rois"].astype(np.float32)
    # the head's boxes: the rois refined a little (so that roi_* and rcnn_* differ)
    u = common._hash01(B * n * 7, salt + 1).reshape(B, n, 7) - np.float32(0.5)
    boxes = (rois + u * np.array([0.4, 0.4, 0.1, 0.2, 0.1, 0.1, 0.1], np.float32)).astype(np.float32)
    if n <= 1024:
        logits = ((common._hash01(B * n * C, salt).reshape(B, n, C) - np.float32(0.5)) * np.float32(8.0)).astype(np.float32)
    else:
        # a seeded permutation of an evenly spaced grid per scene: scores pairwise apart by construction; most of it below the threshold
        rng = np.random.RandomState(LARGE_SEED)
        grid = np.linspace(-14.0, 1.6, n).astype(np.float32)
        logits = np.stack([grid[rng.permutation(n)] for _ in range(B)]).reshape(B, n, 1)
    if c.get("quiet_scene") is not None:
        logits[c["quiet_scene"]] = np.float32(-3.0)
    bd = {"batch_size": B, "batch_box_preds": boxes, "gt_boxes": inp["gt_boxes"].astype(np.float32), "cls_preds_normalized": False}
    if c.get("normalized"):
        bd["batch_cls_preds"] = common._hash01(B * n * C, salt).reshape(B, n, C).astype(np.float32)
        bd["cls_preds_normalized"] = True
    else:
        bd["batch_cls_preds"] = logits
    if c.get("rois"):
        bd["rois"] = rois
    if c.get("labels"):
        bd["has_class_labels"] = True
        lab = (1 + np.floor(common._hash01(B * n, salt + 2) * 3)).astype(np.int64).reshape(B, n)
        if c["labels"] == "roi_labels":
            bd["roi_labels"] = lab
        else:
            bd["batch_pred_labels"] = lab.reshape(B, n, 1)
    return bd, C


def sigmoid32(x):
    """fp32 sigmoid through float64: within an ulp of any correctly rounded fp32 implementation"""
    return (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)


def trimmed_gt(gt):
    """generate_recall_record:562-566: trailing rows that sum to zero go, never the first"""
    k = len(gt) - 1
    while k > 0 and gt[k].sum() == 0:
        k -= 1
    return gt[:k + 1]


def restate(bd, cfg, num_class):
    """numpy restatement -> (scenes, recall): scenes = list of dicts selected (input indices in output order) / scores / labels / iou
    (array or None); recall = the reference's recall_dict"""
    from oracle import oracle as orc
    nms = cfg["NMS_CONFIG"]
    assert not nms["MULTI_CLASSES_NMS"]
    thr = cfg["RECALL_THRESH_LIST"]
    recall = {}
    scenes = []
    for b in range(bd["batch_size"]):
        boxes, src = bd["batch_box_preds"][b], bd["batch_cls_preds"][b]
        prob = src if bd["cls_preds_normalized"] else sigmoid32(src)
        score, label = prob.max(-1), prob.argmax(-1) + 1            # (argmax: the first of equal maxima)
        if bd.get("has_class_labels", False):
            label = bd["roi_labels" if "roi_labels" in bd else "batch_pred_labels"][b].reshape(-1)
        above = np.nonzero(score >= np.float32(cfg["SCORE_THRESH"]))[0]
        sel = np.zeros((0,), np.int64)
        if len(above):
            order = np.argsort(-score[above], kind="stable")[:nms["NMS_PRE_MAXSIZE"]]      # descending, equal scores in ascending index
            cand = above[order]
            keep = orc.nms(boxes[cand][:, :7], -np.arange(len(cand), dtype=np.float32), float(nms["NMS_THRESH"]), None,
                           nms["NMS_TYPE"] == "nms_gpu")
            sel = cand[np.asarray(keep, dtype=np.int64)[:nms["NMS_POST_MAXSIZE"]]]
        out_score = src.max(-1)[sel] if cfg["OUTPUT_RAW_SCORE"] else score[sel]
        iou = None
        if "gt_boxes" in bd:
            if not recall:
                recall = {"gt": 0}
                for t in thr:
                    recall["roi_%s" % t] = 0
                    recall["rcnn_%s" % t] = 0
            gt = trimmed_gt(bd["gt_boxes"][b])
            measured = boxes if "rois" in bd else boxes[sel]
            if len(gt):
                m = orc.boxes_iou3d(measured[:, :7], gt[:, :7]) if len(measured) else np.zeros((0, len(gt)), np.float32)
                r = orc.boxes_iou3d(bd["rois"][b][:, :7], gt[:, :7]) if "rois" in bd else None
                for t in thr:
                    if len(m):
                        recall["rcnn_%s" % t] += int((m.max(0) > t).sum())
                    if r is not None:
                        recall["roi_%s" % t] += int((r.max(0) > t).sum())
                recall["gt"] += len(gt)
                if len(m) and len(m) == len(sel):
                    iou = m.max(1)
        scenes.append({"selected": sel.astype(np.int64), "scores": out_score.astype(np.float32), "labels": np.asarray(label)[sel].astype(np.int64),
                       "iou": iou})
    return scenes, recall


def margins(bd, cfg, sels):
    """the worst distance of the inputs from every threshold a decision crosses -> dict score / gap / nms / recall (oracle arithmetic,
    float64 scores).  score: any score to SCORE_THRESH; gap: two DIFFERENT scores above the threshold (equal scores are a tie, decided by
    index); nms: any candidate pair's IoU to NMS_THRESH; recall: a ground truth's best 3-D IoU (over what the record is taken over:
    every box and roi when rois are given, the selected boxes sels[b] otherwise) to a recall threshold"""
    from oracle import oracle as orc
    nms = cfg["NMS_CONFIG"]
    worst = {"score": 1.0, "gap": 1.0, "nms": 1.0, "recall": 1.0}
    for b in range(bd["batch_size"]):
        src = bd["batch_cls_preds"][b].astype(np.float64)
        prob = src if bd["cls_preds_normalized"] else 1.0 / (1.0 + np.exp(-src))
        score = prob.max(-1)
        if len(score):
            worst["score"] = min(worst["score"], float(np.abs(score - cfg["SCORE_THRESH"]).min()))
        above = np.nonzero(score >= cfg["SCORE_THRESH"])[0]
        d = np.diff(np.sort(score[above]))
        d = d[d > 0]
        if len(d):
            worst["gap"] = min(worst["gap"], float(d.min()))
        cand = above[np.argsort(-score[above], kind="stable")[:nms["NMS_PRE_MAXSIZE"]]]
        boxes = bd["batch_box_preds"][b]
        if len(cand) > 1:
            bx = np.ascontiguousarray(boxes[cand][:, :7])
            if nms["NMS_TYPE"] == "nms_gpu":
                iou = orc.boxes_iou_bev(bx, bx)
            else:
                lo, hi = bx[:, None, 0:2] - bx[:, None, 3:5] / 2, bx[:, None, 0:2] + bx[:, None, 3:5] / 2
                wh = np.clip(np.minimum(hi, hi.transpose(1, 0, 2)) - np.maximum(lo, lo.transpose(1, 0, 2)), 0, None)
                inter = wh[..., 0] * wh[..., 1]
                area = bx[:, 3] * bx[:, 4]
                iou = inter / np.clip(area[:, None] + area[None, :] - inter, 1e-8, None)
            worst["nms"] = min(worst["nms"], float(np.abs(iou[np.triu_indices(len(bx), 1)] - nms["NMS_THRESH"]).min()))
        if "gt_boxes" not in bd:
            continue
        gt = trimmed_gt(bd["gt_boxes"][b])
        for measured in ([boxes, bd["rois"][b]] if "rois" in bd else [boxes[sels[b]]]):
            if len(measured) == 0 or len(gt) == 0:
                continue
            best = orc.boxes_iou3d(measured[:, :7], gt[:, :7]).max(0)
            for t in cfg["RECALL_THRESH_LIST"]:
                worst["recall"] = min(worst["recall"], float(np.abs(best - t).min()))
    return worst


MARGIN = {"score": 1e-5, "gap": 1e-5, "nms": 1e-4, "recall": 2e-4}      # what the golden generator asserts; seeded cases are drawn to it too


def seeded_case(seed, B, n, num_class=1, rois=False, labels=False, normalized=False, logits=(-4.0, 4.0), zero_boxes=0, dup_scores=0, cfg=None, nms=None,
                gt_rows=6):
    """a random batch whose decisions are `MARGIN` away from every threshold: drawn from numpy's RandomState(seed), re-drawn with seed +
    1000 k until the margins hold (so that the GPU may be held to exact decisions against the oracle-based restatement).  Boxes come in
    clusters of about 8 around random objects (they suppress each other); the first objects are the ground truth, zero-padded.
    The logits are a permutation of an evenly spaced grid over `logits` (scores apart by construction; (0.5, 3.5) puts everything above
    a threshold of 0.6, (-6, -1) everything below); zero_boxes: that many all-zero boxes per scene
    (what zero-padded rois decode to); dup_scores: that many boxes per scene share their logits with another box (the tie rule).
    -> (batch_dict of numpy arrays, config dict, restate()'s result)"""
    c = {k: (dict(v) if isinstance(v, dict) else v) for k, v in BASE_CFG.items()}
    c.update(cfg or {})
    c["NMS_CONFIG"].update(nms or {})
    for k in range(50):
        rng = np.random.RandomState(seed + 1000 * k)
        n_obj = max(1, n // 8)
        side = int(np.ceil(np.sqrt(n_obj)))                 # objects on distinct cells of a 12 m lattice: clusters do not meet each other
        cell = np.stack([rng.permutation(side * side)[:n_obj] for _ in range(B)])
        xy = np.stack([cell // side, cell % side - side // 2], axis=2) * 12.0 + 6.0 + rng.uniform(-2, 2, (B, n_obj, 2))
        obj = np.concatenate([xy, rng.uniform(-1.5, -0.5, (B, n_obj, 1)), rng.uniform([3.2, 1.4, 1.3], [4.6, 1.9, 1.8], (B, n_obj, 3)),
                              rng.uniform(-3.1, 3.1, (B, n_obj, 1))], axis=2)
        pick = rng.randint(0, n_obj, (B, n))
        base = np.take_along_axis(obj, pick[..., None], axis=1)
        jit = rng.uniform(-0.5, 0.5, (B, n, 7)) * np.array([2.5, 2.5, 0.4, 0.6, 0.3, 0.3, 0.6])
        boxes = (base + jit).astype(np.float32)
        roi = (boxes + rng.uniform(-0.5, 0.5, (B, n, 7)) * np.array([0.6, 0.6, 0.2, 0.3, 0.2, 0.2, 0.2])).astype(np.float32)
        if zero_boxes:
            boxes[:, n - zero_boxes:] = 0
            roi[:, n - zero_boxes:] = 0
        G = min(gt_rows, n_obj)
        gt = np.zeros((B, G + 2, 8), np.float32)
        gt[:, :G, :7] = obj[:, :G]
        gt[:, :G, 7] = 1
        if B > 1:
            gt[B - 1] = 0                                   # the last scene has no ground truth
        grid = np.linspace(logits[0], logits[1], n * num_class).astype(np.float32)
        lg = np.stack([grid[rng.permutation(n * num_class)] for _ in range(B)]).reshape(B, n, num_class)
        if dup_scores:
            src = rng.randint(0, n, (B, dup_scores))
            dst = rng.randint(0, n, (B, dup_scores))
            for b in range(B):
                lg[b, dst[b]] = lg[b, src[b]]
        bd = {"batch_size": B, "batch_box_preds": boxes, "gt_boxes": gt, "cls_preds_normalized": bool(normalized)}
        bd["batch_cls_preds"] = sigmoid32(lg) if normalized else lg
        if rois:
            bd["rois"] = roi
        if labels:
            bd["has_class_labels"] = True
            bd["roi_labels"] = rng.randint(1, 4, (B, n)).astype(np.int64)
        scenes, recall = restate(bd, c, num_class)
        w = margins(bd, c, [s["selected"] for s in scenes])
        if all(w[key] >= MARGIN[key] for key in MARGIN):
            return bd, c, (scenes, recall)
    raise AssertionError("no draw of seed %d held the margins" % seed)


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_scene(g, name, b):
    """-> dict like restate()'s scenes[b] from the golden file"""
    p = "%s_%d_" % (name, b)
    iou = g[p + "iou"]
    return {"selected": g[p + "selected"].astype(np.int64), "scores": g[p + "scores"], "labels": g[p + "labels"].astype(np.int64),
            "iou": iou if int(g[p + "has_iou"]) else None}


def golden_recall(g, name, cfg):
    c = g[name + "_recall"]
    thr = cfg["RECALL_THRESH_LIST"]
    d = {"gt": int(c[0])}
    for t, th in enumerate(thr):
        d["roi_%s" % th] = int(c[1 + t])
        d["rcnn_%s" % th] = int(c[1 + len(thr) + t])
    return d
