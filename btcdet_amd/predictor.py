"""Inference front end: ``BtcPredictor(model)`` runs the unchanged eval-mode forward of a ``BtcHotPath`` with heads and turns its
``batch_cls_preds`` / ``batch_box_preds`` into detections (btcdet_amd/post_processing.py) -- what a user of the reference gets from
``model(batch)`` in eval mode (btcnet.py:58-66: ``pred_dicts, recall_dicts = self.post_processing(batch_dict)``)."""
import torch

from . import post_processing as pp


class BtcPredictor(object):
    def __init__(self, model, post_cfg=None, num_class=None):
        if getattr(model, "heads", None) not in ("rpn", "full"):
            raise ValueError("BtcPredictor needs a BtcHotPath built with heads='rpn' or 'full' (nothing else produces boxes)")
        self.model = model.eval()
        self.post_cfg = post_cfg if post_cfg is not None else model.cfg.MODEL.POST_PROCESSING
        self.num_class = int(num_class) if num_class is not None else len(model.cfg.CLASS_NAMES)
        if self.post_cfg.NMS_CONFIG.MULTI_CLASSES_NMS:
            raise NotImplementedError("MULTI_CLASSES_NMS")
        self.recall = None       # int64 [gt, roi_t..., rcnn_t...] on the device, accumulated over the calls

    @torch.no_grad()
    def forward(self, batch):
        """prepare(is_train=False) + the model's own forward -> its batch_dict"""
        self.model.eval()
        _, _, batch_dict = self.model(self.model.prepare(batch, is_train=False))
        return batch_dict

    @torch.no_grad()
    def __call__(self, batch):
        """-> post_processing.Detections, resident; the recall record is added to self.recall on the device (no read-back)"""
        batch_dict = self.forward(batch)
        det = pp.detect(batch_dict, self.post_cfg, self.num_class, recall=self.recall)
        if det.recall is not None:
            self.recall = det.recall
        return det

    @torch.no_grad()
    def predict(self, batch):
        """-> (pred_dicts, recall_dict) of this batch as the reference returns them (one read-back); its record also joins self.recall"""
        batch_dict = self.forward(batch)
        det = pp.detect(batch_dict, self.post_cfg, self.num_class)
        if det.recall is not None:
            self.recall = det.recall.clone() if self.recall is None else self.recall + det.recall
        return pp.to_reference(det, batch_dict, self.post_cfg)

    def recall_summary(self):
        """the accumulated record as the reference's recall_dict: reads the counters once"""
        if self.recall is None:
            return {}
        return pp.recall_dict_from(self.recall.cpu().numpy(), self.post_cfg.RECALL_THRESH_LIST)

    def reset_recall(self):
        self.recall = None
