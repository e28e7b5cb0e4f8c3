"""The anchor head's targets and boxes on the GPU (csrc/anchor_targets.hip, include/btcdet_hip_heads.h).

    assigner = DeviceTargetAssigner(model_cfg, class_names, box_coder)        # the signature of dense_head.AxisAlignedTargetAssigner
    targets = assigner.assign_targets(all_anchors, gt_boxes_with_classes)     # the same dict: box_cls_labels, box_reg_targets, reg_weights
    boxes = decode_boxes(box_preds, flat_anchors, dir_cls_preds, model_cfg)   # generate_predicted_boxes' boxes, detached

What is replaced: dense_head.AxisAlignedTargetAssigner.assign_targets -- a Python loop over scenes and anchor-class configurations with
a host read-back per padding row and per configuration, four nonzero calls and a dense (A, G) overlap matrix per call -- by
btc_anchor_targets (three launches for the batch, no read-back, no upload: the configuration tables travel in the kernel arguments), and
ResidualCoder.decode_torch plus the direction-bin correction by btc_decode_anchor_boxes (one launch).

Kept quirks of the reference: row 0 of a scene is kept even when it is padding; class id 0 lands on the LAST class name
(class_names[c - 1]); a forced anchor takes the class of its own best box, not of the box it ties; a box no anchor touches forces
nothing; the smallest box index wins among equal overlaps.

Opt-in: dense_head.AnchorHeadSingle uses this module when TARGET_ASSIGNER_CONFIG.DEVICE is set and `supported` holds; the decoded boxes
then carry no gradient (nothing in the model differentiates through them: proposal_layer runs under no_grad).  There is no CPU
fallback in here: tensors that are not on the GPU raise."""
import numpy as np
import torch

MAX_SLOTS, MAX_CFGS, MAX_CLASSES = 64, 16, 64      # BTC_HEADS_MAX_* of include/btcdet_hip_heads.h


def _get(cfg, key, default=None):
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


def slots_per_config(generator_cfg):
    """anchors per location of each configuration, without the bottom heights: they are the slowest axis of the flat order (nz)"""
    return [len(c["anchor_sizes"]) * len(c["anchor_rotations"]) for c in generator_cfg]


class DeviceTargetAssigner(object):
    @staticmethod
    def unsupported_reason(model_cfg, box_coder, match_height=False):
        """None when btc_anchor_targets computes what AxisAlignedTargetAssigner would, else a sentence naming the option that bars it"""
        gen, tgt = model_cfg.ANCHOR_GENERATOR_CONFIG, model_cfg.TARGET_ASSIGNER_CONFIG
        if _get(tgt, "POS_FRACTION", -1.0) >= 0:
            return "POS_FRACTION >= 0 (random sampling of positives and negatives) is not computed on the device"
        if match_height or _get(tgt, "MATCH_HEIGHT", False):
            return "MATCH_HEIGHT (the rotated 3-D overlap) is not computed on the device"
        if _get(tgt, "NORM_BY_NUM_EXAMPLES", False):
            return "NORM_BY_NUM_EXAMPLES is not computed on the device"
        if _get(model_cfg, "USE_MULTIHEAD", False):
            return "USE_MULTIHEAD is not computed on the device"
        if getattr(box_coder, "encode_angle_by_sincos", False):
            return "encode_angle_by_sincos is not computed on the device"
        if getattr(box_coder, "code_size", 7) != 7:
            return "a box code size of %d (not 7) is not computed on the device" % box_coder.code_size
        if len({len(c["anchor_rotations"]) for c in gen}) != 1:
            return "ANCHOR_GENERATOR_CONFIG entries with different numbers of anchor_rotations have no common flat anchor order"
        if len({len(c["anchor_bottom_heights"]) for c in gen}) != 1:
            return "ANCHOR_GENERATOR_CONFIG entries with different numbers of anchor_bottom_heights have no common flat anchor order"
        names = [c["class_name"] for c in gen]
        if len(set(names)) != len(names):
            return "two ANCHOR_GENERATOR_CONFIG entries of one class_name cannot share the class table"
        if sum(slots_per_config(gen)) > MAX_SLOTS or len(gen) > MAX_CFGS:
            return "more than %d anchors per location or %d ANCHOR_GENERATOR_CONFIG entries do not fit the kernel's tables" % (MAX_SLOTS, MAX_CFGS)
        return None

    @staticmethod
    def supported(model_cfg, box_coder):
        return DeviceTargetAssigner.unsupported_reason(model_cfg, box_coder) is None

    def __init__(self, model_cfg, class_names, box_coder, match_height=False):
        why = self.unsupported_reason(model_cfg, box_coder, match_height)
        if why is not None:
            raise ValueError("DeviceTargetAssigner: " + why)
        if len(class_names) >= MAX_CLASSES:
            raise ValueError("DeviceTargetAssigner: %d class_names do not fit the kernel's class table (%d)" % (len(class_names), MAX_CLASSES))
        gen = model_cfg.ANCHOR_GENERATOR_CONFIG
        self.box_coder, self.match_height = box_coder, False
        self.class_names = np.array(class_names)
        self.anchor_class_names = [c["class_name"] for c in gen]
        # the host tables of btc_anchor_targets, built once
        self.slot_cfg = np.ascontiguousarray(np.repeat(np.arange(len(gen)), slots_per_config(gen)).astype(np.int32))
        self.matched = np.array([c["matched_threshold"] for c in gen], dtype=np.float32)
        self.unmatched = np.array([c["unmatched_threshold"] for c in gen], dtype=np.float32)
        # class id c -> class_names[c - 1] -> its configuration; c = 0 wraps to the last name, as the reference's indexing does
        self.class_cfg = np.array([self.anchor_class_names.index(self.class_names[c - 1]) if self.class_names[c - 1] in self.anchor_class_names else -1
                                   for c in range(len(class_names) + 1)], dtype=np.int32)
        self._flat = {}

    def flat_anchors(self, all_anchors):
        """(A, 7) anchors in the head's _flat_anchors order, cached per device and anchor list"""
        key = (str(all_anchors[0].device),) + tuple(a.data_ptr() for a in all_anchors)
        hit = self._flat.get(key)
        if hit is None:
            if len(all_anchors) != len(self.anchor_class_names):
                raise ValueError("DeviceTargetAssigner: %d anchor tensors for %d configurations" % (len(all_anchors), len(self.anchor_class_names)))
            if len({tuple(a.shape[:3]) for a in all_anchors}) != 1:
                raise ValueError("DeviceTargetAssigner: the configurations' anchor grids differ: %r" % [tuple(a.shape) for a in all_anchors])
            per = [int(a.shape[3] * a.shape[4]) for a in all_anchors]
            if per != [int(n) for n in np.bincount(self.slot_cfg, minlength=len(per))] or any(a.shape[-1] != 7 for a in all_anchors):
                raise ValueError("DeviceTargetAssigner: anchor tensors %r do not match ANCHOR_GENERATOR_CONFIG" % [tuple(a.shape) for a in all_anchors])
            flat = torch.cat(list(all_anchors), dim=-3).reshape(-1, 7).float().contiguous()
            hit = self._flat[key] = (flat, list(all_anchors))      # the list keeps the keyed addresses alive
        return hit[0]

    def assign_targets(self, all_anchors, gt_boxes_with_classes):
        """all_anchors: list per class config of [nz, ny, nx, n_size, n_rot, 7]; gt (B, M, 8) float32 on the GPU, zero rows pad the tail
        -> box_cls_labels (B, A) int32 (-1 ignore, 0 background, class id), box_reg_targets (B, A, 7), reg_weights (B, A).
        Only enqueues on the current stream: no read-back, no upload, no synchronisation."""
        from ._lib import check, lib, ptr, stream_ptr, workspace
        L = lib()
        anchors = self.flat_anchors(all_anchors)
        gt = gt_boxes_with_classes
        if gt.dim() != 3 or gt.shape[-1] != 8 or gt.dtype != torch.float32:
            raise ValueError("DeviceTargetAssigner: gt boxes must be (B, M, 8) float32, got %r %s" % (tuple(gt.shape), gt.dtype))
        if gt.device != anchors.device:
            raise ValueError("DeviceTargetAssigner: boxes on %s, anchors on %s" % (gt.device, anchors.device))
        gt = gt.detach().contiguous()
        B, M, A, dev = int(gt.shape[0]), int(gt.shape[1]), int(anchors.shape[0]), anchors.device
        labels = torch.empty((B, A), dtype=torch.int32, device=dev)
        targets = torch.empty((B, A, 7), dtype=torch.float32, device=dev)
        weights = torch.empty((B, A), dtype=torch.float32, device=dev)
        ws_bytes = L.btc_anchor_targets_ws_bytes(B, M)
        ws = workspace(ws_bytes, dev)
        check(L.btc_anchor_targets(ptr(anchors) if A else None, A, int(self.slot_cfg.shape[0]), self.slot_cfg.ctypes.data, int(self.matched.shape[0]),
                                   self.matched.ctypes.data, self.unmatched.ctypes.data, self.class_cfg.ctypes.data, int(self.class_cfg.shape[0]) - 1,
                                   ptr(gt) if M else None, B, M, ptr(labels) if A else None, ptr(targets) if A else None,
                                   ptr(weights) if A else None, ptr(ws), ws_bytes, stream_ptr()), "btc_anchor_targets")
        return {"box_cls_labels": labels, "box_reg_targets": targets, "reg_weights": weights}


def decode_boxes(box_preds, anchors, dir_cls_preds, cfg):
    """box_preds (B, A, 7), anchors (A, 7), dir_cls_preds (B, A, NUM_DIR_BINS) or None, cfg with DIR_OFFSET, DIR_LIMIT_OFFSET and
    NUM_DIR_BINS -> boxes (B, A, 7), detached: ResidualCoder.decode_torch and the direction-bin correction in one launch"""
    from ._lib import check, lib, ptr, stream_ptr
    if box_preds.dim() != 3 or box_preds.shape[-1] != 7 or anchors.dim() != 2 or tuple(anchors.shape) != (box_preds.shape[1], 7):
        raise ValueError("decode_boxes: box_preds %r against anchors %r" % (tuple(box_preds.shape), tuple(anchors.shape)))
    if box_preds.dtype != torch.float32 or anchors.dtype != torch.float32:
        raise ValueError("decode_boxes: float32 only, got %s and %s" % (box_preds.dtype, anchors.dtype))
    preds = box_preds.detach().contiguous()
    anchors = anchors.contiguous()
    B, A = int(preds.shape[0]), int(preds.shape[1])
    dirs, bins, off, lim = None, 0, 0.0, 0.0
    if dir_cls_preds is not None:
        bins, off, lim = int(_get(cfg, "NUM_DIR_BINS")), float(_get(cfg, "DIR_OFFSET")), float(_get(cfg, "DIR_LIMIT_OFFSET"))
        if tuple(dir_cls_preds.shape) != (B, A, bins) or dir_cls_preds.dtype != torch.float32:
            raise ValueError("decode_boxes: dir_cls_preds %r %s against (%d, %d, %d) float32" % (tuple(dir_cls_preds.shape), dir_cls_preds.dtype, B, A, bins))
        dirs = dir_cls_preds.detach().contiguous()
    boxes = torch.empty((B, A, 7), dtype=torch.float32, device=preds.device)
    check(lib().btc_decode_anchor_boxes(ptr(preds) if A else None, ptr(anchors) if A else None, ptr(dirs) if (dirs is not None and A) else None, B, A,
                                        bins, off, lim, ptr(boxes) if A else None, stream_ptr()), "btc_decode_anchor_boxes")
    return boxes
