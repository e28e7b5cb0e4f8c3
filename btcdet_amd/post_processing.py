"""Detections from the eval-mode head outputs: the reference's ``Detector3DTemplate.post_processing``
(detector3d_template.py:363-476 with model_nms_utils.class_agnostic_nms and generate_recall_record, :548-591) on the device.

The reference walks the scenes in Python: sigmoid, max, mask, ``nonzero``, ``topk``, an NMS with a host-side keep list, two IoU matrices
and one ``.item()`` per recall threshold.  Here a batch is

* ``n <= 1024`` boxes per scene (behind the ROI head: its NMS_PRE_MAXSIZE at test time bounds n): two launches of libbtcdet_hip.so,
  ``btc_det_select_nms`` and ``btc_det_finish`` (csrc/det_post.hip);
* more (straight behind the anchor head): the scores masked and sorted by torch, ``iou3d_nms.nms_topk``, then ``btc_det_finish``;

and nothing is read back: ``detect`` returns padded tensors and device counters.  ``post_processing`` gives the reference's return
value from them with ONE copy to the host per batch.  There is no fallback: a missing kernel is an error."""
import ctypes
from collections import namedtuple

import torch

from . import iou3d_nms
from ._lib import c_f32p, check, lib, ptr, stream_ptr, workspace

FUSED_MAX_BOXES = 1024     # btc_det_select_nms: candidates per scene
MAX_THRESHOLDS = 8

# boxes (B, K, D), scores (B, K), labels (B, K) int64, num (B,) int32, iou (B, K), recall int64 [1 + 2T] or None -- K = NMS_POST_MAXSIZE,
# rows past num[b] are zeros; with_rois: whether iou / rcnn_* are over the INPUT boxes (the reference's choice when `rois` is given)
Detections = namedtuple("Detections", ["boxes", "scores", "labels", "num", "iou", "recall", "thresholds", "with_rois", "num_boxes"])


def new_recall(thresh_list, device):
    """the recall record on the device: int64 [gt, roi_t..., rcnn_t...], added to by every detect() it is handed to"""
    if len(thresh_list) > MAX_THRESHOLDS:
        raise ValueError("at most %d recall thresholds, got %d" % (MAX_THRESHOLDS, len(thresh_list)))
    return torch.zeros((1 + 2 * len(thresh_list),), dtype=torch.int64, device=device)


def recall_dict_from(counters, thresh_list):
    """host counters [1 + 2T] -> the reference's recall_dict ('gt', 'roi_0.3', 'rcnn_0.3', ...)"""
    T = len(thresh_list)
    d = {"gt": int(counters[0])}
    for t, th in enumerate(thresh_list):
        d["roi_%s" % str(th)] = int(counters[1 + t])
        d["rcnn_%s" % str(th)] = int(counters[1 + T + t])
    return d


def _inputs(batch_dict, post_cfg, num_class):
    nms = post_cfg.NMS_CONFIG
    if nms.MULTI_CLASSES_NMS:
        raise NotImplementedError("MULTI_CLASSES_NMS")
    if nms.NMS_TYPE not in ("nms_gpu", "nms_normal_gpu"):
        raise NotImplementedError("NMS_TYPE %r" % (nms.NMS_TYPE,))
    cls, boxes = batch_dict["batch_cls_preds"], batch_dict["batch_box_preds"]
    if isinstance(cls, (list, tuple)):
        raise NotImplementedError("a list of batch_cls_preds (multi-head) needs MULTI_CLASSES_NMS")
    if batch_dict.get("batch_index", None) is not None or boxes.dim() != 3:
        raise NotImplementedError("stacked 2-D batch_box_preds with batch_index")
    B = int(batch_dict["batch_size"])
    assert boxes.shape[0] == B and cls.shape[0] == B and cls.shape[1] == boxes.shape[1]
    assert cls.shape[2] in (1, num_class), "batch_cls_preds has %d classes, expected 1 or %d" % (cls.shape[2], num_class)
    assert boxes.shape[2] >= 7
    return cls.detach().float().contiguous(), boxes.detach().float().contiguous(), B


@torch.no_grad()
def detect(batch_dict, post_cfg, num_class, recall=None, path=None):
    """-> Detections, all resident on the device, nothing read back.

    recall: the int64 counters of new_recall() to ADD this batch's record to (one tensor accumulates over an evaluation run); None: a
    fresh one when the batch has `gt_boxes`.  path: None (by n), "fused" (n <= 1024 only) or "large"."""
    cls, boxes, B = _inputs(batch_dict, post_cfg, num_class)
    nms = post_cfg.NMS_CONFIG
    n, C, D = int(cls.shape[1]), int(cls.shape[2]), int(boxes.shape[2])
    K, pre = int(nms.NMS_POST_MAXSIZE), int(nms.NMS_PRE_MAXSIZE)
    dev = boxes.device
    normalized = bool(batch_dict["cls_preds_normalized"])
    raw = bool(post_cfg.get("OUTPUT_RAW_SCORE", False))
    rotated = nms.NMS_TYPE == "nms_gpu"
    thresholds = [float(t) for t in post_cfg.RECALL_THRESH_LIST]
    if len(thresholds) > MAX_THRESHOLDS:
        raise ValueError("at most %d recall thresholds, got %d" % (MAX_THRESHOLDS, len(thresholds)))
    if path is None:
        path = "fused" if n <= FUSED_MAX_BOXES else "large"
    assert path in ("fused", "large"), path
    L = lib()
    if path == "fused":
        keep = torch.empty((B, K), dtype=torch.int64, device=dev)
        num = torch.empty((B,), dtype=torch.int32, device=dev)
        best_class = torch.empty((B, n), dtype=torch.int32, device=dev)
        ws_bytes = L.btc_det_select_nms_ws_bytes(B, n)
        ws = workspace(ws_bytes, dev)
        check(L.btc_det_select_nms(ptr(cls), ptr(boxes), B, n, C, D, int(normalized), float(post_cfg.SCORE_THRESH), float(nms.NMS_THRESH), int(rotated),
                                   pre, K, ptr(keep), ptr(num), ptr(best_class), ptr(ws), ws_bytes, stream_ptr()), "btc_det_select_nms")
    else:
        # scores below the threshold (and NaN) -> -inf: they sort behind every valid candidate and cannot suppress one, so the valid
        # detections are the prefix of the kept list whose score passed -- what the reference computes on the masked subset.  A STABLE
        # descending sort instead of torch.topk: equal scores go in ascending input index, as in the fused kernel.
        prob = cls if normalized else torch.sigmoid(cls)
        best, best_class = torch.max(prob, dim=2)
        neg = torch.full_like(best, float("-inf"))
        masked = torch.where(best >= float(post_cfg.SCORE_THRESH), best, neg)
        k = min(pre, n)
        top_scores, top = torch.sort(masked, dim=1, descending=True, stable=True)
        top_scores, top = top_scores[:, :k], top[:, :k]
        cand = torch.gather(boxes[..., 0:7], 1, top.unsqueeze(-1).expand(-1, -1, 7)).contiguous()
        kpos, _ = iou3d_nms.nms_topk(cand, float(nms.NMS_THRESH), K, rotated=rotated)
        pos = kpos.clamp(min=0)
        valid = (kpos >= 0) & (torch.gather(top_scores, 1, pos) > float("-inf"))
        keep = torch.where(valid, torch.gather(top, 1, pos), torch.full_like(kpos, -1))
        num = valid.sum(dim=1).to(torch.int32)
        best_class = best_class.to(torch.int32).contiguous()
    labels = None
    if batch_dict.get("has_class_labels", False):
        labels = batch_dict["roi_labels" if "roi_labels" in batch_dict else "batch_pred_labels"]
        labels = labels.reshape(B, n).to(torch.int64).contiguous()
    gt = batch_dict.get("gt_boxes", None)
    rois = batch_dict.get("rois", None)
    if gt is not None:
        gt = gt.detach().float().contiguous()
        if recall is None:
            recall = new_recall(thresholds, dev)
        assert recall.dtype == torch.int64 and recall.numel() == 1 + 2 * len(thresholds) and recall.is_contiguous()
    if rois is not None:
        rois = rois.detach().float().contiguous()
    out_boxes = torch.empty((B, K, D), dtype=torch.float32, device=dev)
    out_scores = torch.empty((B, K), dtype=torch.float32, device=dev)
    out_labels = torch.empty((B, K), dtype=torch.int64, device=dev)
    out_iou = torch.empty((B, K), dtype=torch.float32, device=dev)
    h_thr = (ctypes.c_float * max(len(thresholds), 1))(*thresholds)
    check(L.btc_det_finish(ptr(cls), ptr(boxes), B, n, C, D, int(normalized), int(raw), ptr(keep), ptr(num), ptr(best_class), ptr(labels), K,
                           ptr(gt), 0 if gt is None else int(gt.shape[1]), 0 if gt is None else int(gt.shape[2]),
                           ptr(rois), 0 if rois is None else int(rois.shape[1]), 0 if rois is None else int(rois.shape[2]),
                           ctypes.cast(h_thr, c_f32p), len(thresholds), ptr(out_boxes), ptr(out_scores), ptr(out_labels), ptr(out_iou),
                           ptr(recall) if gt is not None else None, stream_ptr()), "btc_det_finish")
    return Detections(out_boxes, out_scores, out_labels, num, out_iou, recall if gt is not None else None, thresholds,
                      rois is not None, n)


@torch.no_grad()
def post_processing(batch_dict, post_cfg, num_class, path=None):
    """-> (pred_dicts, recall_dict) with the reference's shapes and keys, from detect() with ONE read-back per batch (counts, counters
    and the IoU column in a single copy).  pred_boxes / pred_scores / pred_labels stay on the device (views of the padded outputs);
    `iou` is a numpy array or None exactly where the reference returns None."""
    return to_reference(detect(batch_dict, post_cfg, num_class, path=path), batch_dict, post_cfg)


def to_reference(det, batch_dict, post_cfg):
    """Detections of detect(batch_dict, ...) with a record of its own -> the reference's (pred_dicts, recall_dict): the one read-back"""
    B, K = det.scores.shape
    has_gt = det.recall is not None
    n_gt = int(batch_dict["gt_boxes"].shape[1]) if has_gt else 0
    parts = [det.num.to(torch.float64)]
    if has_gt:
        parts += [det.recall.to(torch.float64), det.iou.reshape(-1).to(torch.float64)]      # (exact: int32 counts, float32 IoUs, counters < 2^53)
    host = torch.cat(parts).cpu().numpy()                                                     # the read-back
    nums = host[:B].astype("int64")
    recall_dict = {}
    iou = None
    if has_gt:
        T = len(det.thresholds)
        recall_dict = recall_dict_from(host[B:B + 1 + 2 * T].astype("int64"), post_cfg.RECALL_THRESH_LIST)
        iou = host[B + 1 + 2 * T:].astype("float32").reshape(B, K)
    pred_dicts = []
    for b in range(B):
        k = int(nums[b])
        scene_iou = None
        if iou is not None and n_gt > 0:
            rows = det.num_boxes if det.with_rois else k       # rows of the IoU matrix the reference built
            if rows > 0 and rows == k:
                scene_iou = iou[b, :k].copy()
        pred_dicts.append({"pred_boxes": det.boxes[b, :k], "pred_scores": det.scores[b, :k], "pred_labels": det.labels[b, :k], "iou": scene_iou})
    return pred_dicts, recall_dict
