"""Inference front end: ``BtcPredictor(model)`` runs the unchanged eval-mode forward of a ``BtcHotPath`` with heads and turns its
``batch_cls_preds`` / ``batch_box_preds`` into detections (btcdet_amd/post_processing.py) -- what a user of the reference gets from
``model(batch)`` in eval mode (btcnet.py:58-66: ``pred_dicts, recall_dicts = self.post_processing(batch_dict)``).  With
``occ_metrics=True`` the occupancy metrics of the batch (btcdet_amd/occ_metrics.py; btcnet.py:70-73, which the reference runs when its
configuration carries MODEL.OCC.OCC_POST_PROCESSING) are gathered as well."""
import torch

from . import occ_metrics as om
from . import post_processing as pp


class BtcPredictor(object):
    def __init__(self, model, post_cfg=None, num_class=None, occ_metrics=False):
        if getattr(model, "heads", None) not in ("rpn", "full"):
            raise ValueError("BtcPredictor needs a BtcHotPath built with heads='rpn' or 'full' (nothing else produces boxes)")
        self.model = model.eval()
        self.post_cfg = post_cfg if post_cfg is not None else model.cfg.MODEL.POST_PROCESSING
        self.num_class = int(num_class) if num_class is not None else len(model.cfg.CLASS_NAMES)
        if self.post_cfg.NMS_CONFIG.MULTI_CLASSES_NMS:
            raise NotImplementedError("MULTI_CLASSES_NMS")
        self.recall = None       # int64 [gt, roi_t..., rcnn_t...] on the device, accumulated over the calls
        self.occ = om.OccEvaluator() if occ_metrics else None       # one row of 16 counters per batch, on the device

    @torch.no_grad()
    def forward(self, batch):
        """prepare(is_train=False) + the model's own forward -> its batch_dict"""
        self.model.eval()
        _, _, batch_dict = self.model(self.model.prepare(batch, is_train=False))
        return batch_dict

    @torch.no_grad()
    def __call__(self, batch):
        """-> post_processing.Detections, resident; the recall record is added to self.recall on the device (no read-back), and with
        occ_metrics the batch's occupancy counters to self.occ"""
        batch_dict = self.forward(batch)
        if self.occ is not None:
            self.occ.add(batch_dict)
        det = pp.detect(batch_dict, self.post_cfg, self.num_class, recall=self.recall)
        if det.recall is not None:
            self.recall = det.recall
        return det

    @torch.no_grad()
    def predict(self, batch):
        """-> (pred_dicts, recall_dict) of this batch as the reference returns them (one read-back); its record also joins self.recall.
        With occ_metrics the batch's row joins self.occ and its match_dicts are merged into the returned dict, the recall entries on
        top, as btcnet.py:70-86 does (one more read-back, of 16 counters)"""
        batch_dict = self.forward(batch)
        det = pp.detect(batch_dict, self.post_cfg, self.num_class)
        if det.recall is not None:
            self.recall = det.recall.clone() if self.recall is None else self.recall + det.recall
        pred_dicts, recall_dict = pp.to_reference(det, batch_dict, self.post_cfg)
        if self.occ is None:
            return pred_dicts, recall_dict
        metric_dict = om.match_dicts_from(self.occ.add(batch_dict).cpu(), with_boxes="occ_pnts" in batch_dict)
        metric_dict.update(recall_dict)
        return pred_dicts, metric_dict

    def recall_summary(self):
        """the accumulated record as the reference's recall_dict: reads the counters once"""
        if self.recall is None:
            return {}
        return pp.recall_dict_from(self.recall.cpu().numpy(), self.post_cfg.RECALL_THRESH_LIST)

    def reset_recall(self):
        self.recall = None

    def occ_summary(self):
        """the occupancy metrics accumulated over the calls (OccEvaluator.summary: reads the table once); {} without occ_metrics"""
        return self.occ.summary() if self.occ is not None else {}
