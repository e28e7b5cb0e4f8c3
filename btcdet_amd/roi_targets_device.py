"""The ROI head's training targets on the GPU (csrc/roi_targets.hip, include/btcdet_hip_roi_targets.h): one launch per batch.

    targets = DeviceProposalTargets(model_cfg.ROI_HEAD.TARGET_CONFIG)(batch_dict)

What is replaced: roi_targets.ProposalTargetLayer.forward followed by roi_targets.canonical_targets -- per scene a pairwise-overlap launch,
a dozen elementwise launches for the 3-D IoU, a masked max, three sorts, a dozen `where`s and five gathers, then the stacks, the label
arithmetic and the canonical transform -- by btc_roi_targets.  The returned dict has the torch route's keys, shapes and dtypes (a consumer
cannot tell the routes apart) plus `max_overlaps`, `gt_assignment` and `sampled_inds`.  The inputs are what proposal_layer leaves (float32
rois and scores, int64 labels); nothing is converted, read back or synchronised.

Sampling: ONE `torch.rand((B, 4, M))`, M = max(ROI_PER_IMAGE, N), per batch from a generator on the device; the kernel samples from it as
roi_targets.sample_rois does from its per-scene (4, M) draw -- the same distribution, another random stream (as sample_rois says of itself
against the reference).  `uniforms=` / `sampled_inds=` hand the uniforms or the draw itself over (tests: equal draws on both routes).

Opt-in: conv_head.ConvHead.assign_targets uses this module when ROI_HEAD.TARGET_CONFIG.DEVICE is set and `unsupported_reason` is None.  A
call whose tensors are not float32 / int64 on the GPU, or whose rois are not 7 wide, takes the torch route for that call -- `usable`
decides.  There is no CPU fallback in here: CPU tensors raise."""
import torch

from .anchor_targets import _get

MAX_N, MAX_R = 1024, 1024           # BTC_ROI_TARGETS_MAX_N, BTC_ROI_TARGETS_MAX_R of include/btcdet_hip_roi_targets.h
SCORE_TYPES = {"roi_iou": 0, "cls": 1}   # BTC_ROI_SCORE_ROI_IOU, BTC_ROI_SCORE_CLS

_WS = {}


def unsupported_reason(cfg):
    """None when btc_roi_targets computes what the torch route would, else a sentence naming the option that bars it"""
    R = int(_get(cfg, "ROI_PER_IMAGE", 0))
    if not 1 <= R <= MAX_R:
        return "ROI_PER_IMAGE %d does not fit the kernel's limit (1 <= R <= %d)" % (R, MAX_R)
    if _get(cfg, "CLS_SCORE_TYPE", None) not in SCORE_TYPES:
        return "CLS_SCORE_TYPE %r is not computed on the device" % (_get(cfg, "CLS_SCORE_TYPE", None),)
    return None


def usable(batch_dict):
    """this call's tensors are what the kernel takes: on the GPU, float32 (labels int64), rois 7 wide, boxes 8 wide, N within the limit"""
    rois, scores, labels, gts = (batch_dict.get(k) for k in ("rois", "roi_scores", "roi_labels", "gt_boxes"))
    if any(t is None or not t.is_cuda for t in (rois, scores, labels, gts)):
        return False
    if rois.dtype != torch.float32 or scores.dtype != torch.float32 or gts.dtype != torch.float32 or labels.dtype != torch.int64:
        return False
    return rois.dim() == 3 and rois.shape[-1] == 7 and gts.dim() == 3 and gts.shape[-1] == 8 and 1 <= rois.shape[1] <= MAX_N and gts.shape[1] >= 1 \
        and rois.shape[0] >= 1


def _workspace(nbytes, device, stream):
    """per (device, stream): allocated through _lib.workspace and zeroed ONCE -- every call leaves its counters zero"""
    from ._lib import workspace
    key = (device.index, stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = workspace(max(nbytes, 1 << 16), device)
        ws.zero_()
    return ws


def config_block(cfg):
    """the host struct of the C ABI from a TARGET_CONFIG: thresholds rounded to float32, quota and span formed here"""
    from ._lib import BtcRoiTargetsConfig
    R = int(cfg.ROI_PER_IMAGE)
    return BtcRoiTargetsConfig(R=R, fg_quota=int(round(float(cfg.FG_RATIO) * R)), by_class=int(bool(_get(cfg, "SAMPLE_ROI_BY_EACH_CLASS", False))),
                               score_type=SCORE_TYPES[cfg.CLS_SCORE_TYPE], reg_fg=float(cfg.REG_FG_THRESH), cls_fg=float(cfg.CLS_FG_THRESH),
                               cls_bg=float(cfg.CLS_BG_THRESH), cls_bg_lo=float(cfg.CLS_BG_THRESH_LO),
                               fg_thresh=float(min(cfg.REG_FG_THRESH, cfg.CLS_FG_THRESH)), cls_span=float(cfg.CLS_FG_THRESH) - float(cfg.CLS_BG_THRESH),
                               hard_bg_ratio=float(cfg.HARD_BG_RATIO))


class DeviceProposalTargets(torch.nn.Module):
    """rois (B, N, 7), roi_scores, roi_labels, gt_boxes (B, G, 8) -> canonical_targets(ProposalTargetLayer(...)(...)) in one launch"""

    unsupported_reason = staticmethod(unsupported_reason)
    usable = staticmethod(usable)

    def __init__(self, roi_sampler_cfg, seed=0):
        super().__init__()
        why = unsupported_reason(roi_sampler_cfg)
        if why is not None:
            raise ValueError("DeviceProposalTargets: " + why)
        self.roi_sampler_cfg = roi_sampler_cfg
        self.seed = seed
        self._gen = None
        self._block = config_block(roi_sampler_cfg)

    def _generator(self, device):
        if self._gen is None or self._gen.device != device:
            self._gen = torch.Generator(device=device)
            self._gen.manual_seed(self.seed)
        return self._gen

    @torch.no_grad()
    def forward(self, batch_dict, sampled_inds=None, uniforms=None):
        """sampled_inds (B, R) int64: use these roi indices instead of drawing; uniforms (B, 4, max(R, N)) float32: sample from these"""
        import ctypes
        from ._lib import check, lib, ptr, stream_ptr
        if not usable(batch_dict):
            raise ValueError("DeviceProposalTargets: float32 rois (B, N <= %d, 7), scores and boxes (B, G, 8) and int64 labels on the GPU only "
                             "(there is no CPU fallback in here)" % MAX_N)
        if sampled_inds is not None and uniforms is not None:
            raise ValueError("DeviceProposalTargets: sampled_inds or uniforms, not both")
        rois, scores = batch_dict["rois"].contiguous(), batch_dict["roi_scores"].contiguous()
        labels, gts = batch_dict["roi_labels"].contiguous(), batch_dict["gt_boxes"].contiguous()
        B, N, G = int(rois.shape[0]), int(rois.shape[1]), int(gts.shape[1])
        R = int(self._block.R)
        M = max(R, N)
        dev = rois.device
        if tuple(scores.shape) != (B, N) or tuple(labels.shape) != (B, N) or gts.shape[0] != B:
            raise ValueError("DeviceProposalTargets: shapes rois %r scores %r labels %r boxes %r" % tuple(tuple(t.shape) for t in (rois, scores, labels, gts)))
        if sampled_inds is not None:
            sampled_inds = sampled_inds.contiguous()
            if tuple(sampled_inds.shape) != (B, R) or sampled_inds.dtype != torch.int64 or sampled_inds.device != dev:
                raise ValueError("DeviceProposalTargets: sampled_inds must be (%d, %d) int64 on %s" % (B, R, dev))
        else:
            if uniforms is None:
                uniforms = torch.rand((B, 4, M), device=dev, generator=self._generator(dev))
            uniforms = uniforms.contiguous()
            if tuple(uniforms.shape) != (B, 4, M) or uniforms.dtype != torch.float32 or uniforms.device != dev:
                raise ValueError("DeviceProposalTargets: uniforms must be (%d, 4, %d) float32 on %s" % (B, M, dev))
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)       # (the kernel writes every element: no fills)
        i64 = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
        roi_iou = self._block.score_type == SCORE_TYPES["roi_iou"]
        t = {"rois": f32(B, R, 7), "gt_of_rois": f32(B, R, 8), "gt_of_rois_src": f32(B, R, 8), "gt_iou_of_rois": f32(B, R), "roi_scores": f32(B, R),
             "roi_labels": i64(B, R), "reg_valid_mask": i64(B, R), "rcnn_cls_labels": f32(B, R) if roi_iou else i64(B, R),
             "max_overlaps": f32(B, N), "gt_assignment": i64(B, N), "sampled_inds": i64(B, R)}
        L = lib()
        stream = stream_ptr()
        ws_bytes = int(L.btc_roi_targets_ws_bytes(B, N))
        ws = _workspace(ws_bytes, dev, stream)
        check(L.btc_roi_targets(ptr(rois), ptr(scores), ptr(labels), ptr(gts), ptr(uniforms), ptr(sampled_inds), B, N, G, ctypes.byref(self._block),
                                ptr(t["rois"]), ptr(t["gt_of_rois"]), ptr(t["gt_of_rois_src"]), ptr(t["gt_iou_of_rois"]), ptr(t["roi_scores"]),
                                ptr(t["roi_labels"]), ptr(t["reg_valid_mask"]), ptr(t["rcnn_cls_labels"]), ptr(t["max_overlaps"]),
                                ptr(t["gt_assignment"]), ptr(t["sampled_inds"]), ptr(ws), ws_bytes, stream), "btc_roi_targets")
        return t
