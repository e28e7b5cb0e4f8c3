"""The ROI head's loss on the GPU (csrc/roi_loss.hip, include/btcdet_hip_roi_loss.h): forward one launch, backward one launch.

    total, parts = roi_loss(forward_ret_dict, LOSS_CONFIG.LOSS_WEIGHTS, with_corner=LOSS_CONFIG.CORNER_LOSS_REGULARIZATION)
    # total: rcnn_loss, differentiable with respect to rcnn_cls and rcnn_reg; parts (5): cls, reg, corner, reg + corner, total -- not differentiable

What is replaced: conv_head.ConvHead.get_loss in its torch formulation (roi_targets.rcnn_cls_loss / rcnn_reg_loss) -- a sigmoid and a
binary cross-entropy, two clones with in-place edits, ResidualCoder.encode_torch and decode_torch, a rotation, three corner expansions,
two norms, a min, two smooth-L1s and masked sums, and an autograd twin for each -- by btc_roi_loss_fwd and btc_roi_loss_bwd.  The inputs
are exactly what DeviceProposalTargets (or ProposalTargetLayer + canonical_targets: the dtypes agree) leaves on the device; nothing is
converted, read back or synchronised, and the sums are deterministic.

Kept from the torch route: the clamp of binary_cross_entropy at -100, the normalisers max(#valid, 1) and max(#foreground, 1) over the
whole batch, no code weights, a NaN regression target contributes nothing, the UNCLAMPED roi dims in the corner term's decode.
Different: on an exact tie of a corner's two distances the unflipped box takes the whole gradient (torch's min splits it in half).

Opt-in: ConvHead.get_loss uses this module when ROI_HEAD.LOSS_CONFIG.DEVICE is set and `unsupported_reason` is None.  A call whose
tensors are not on the GPU or not float32 (mask int64, labels float32 or int64) takes the torch route for that call -- `usable`
decides.  There is no CPU fallback in here: roi_loss() on CPU tensors raises."""
import torch

from .anchor_targets import _get

THREADS, LANES, MAX_TILES = 256, 1, 512     # BTC_ROI_LOSS_THREADS, BTC_ROI_LOSS_LANES, BTC_ROI_LOSS_MAX_TILES of include/btcdet_hip_roi_loss.h
LABEL_KINDS = {torch.float32: 0, torch.int64: 1}   # BTC_ROI_SCORE_ROI_IOU, BTC_ROI_SCORE_CLS
KEYS = ("rcnn_cls", "rcnn_reg", "rois", "gt_of_rois", "gt_of_rois_src", "reg_valid_mask", "rcnn_cls_labels")

_WS = {}


def unsupported_reason(loss_cfg, box_coder):
    """None when btc_roi_loss_* computes what the torch route of ConvHead.get_loss would, else a sentence naming the option that bars it"""
    if _get(loss_cfg, "CLS_LOSS", None) != "BinaryCrossEntropy":
        return "CLS_LOSS %r (not BinaryCrossEntropy) is not computed on the device" % (_get(loss_cfg, "CLS_LOSS", None),)
    if _get(loss_cfg, "REG_LOSS", None) != "smooth-l1":
        return "REG_LOSS %r (not smooth-l1) is not computed on the device" % (_get(loss_cfg, "REG_LOSS", None),)
    if getattr(box_coder, "encode_angle_by_sincos", False):
        return "encode_angle_by_sincos is not computed on the device"
    if getattr(box_coder, "code_size", 7) != 7:
        return "a box code size of %d (not 7) is not computed on the device" % box_coder.code_size
    return None


def usable(ret):
    """this call's tensors are what the kernels take: on the GPU, float32 (mask int64, labels float32 or int64), rois 7 wide, boxes >= 7 wide"""
    t = [ret.get(k) for k in KEYS]
    if any(v is None or not v.is_cuda for v in t):
        return False
    cls, reg, rois, gt, src, mask, labels = t
    if any(v.dtype != torch.float32 for v in (cls, reg, rois, gt, src)) or mask.dtype != torch.int64 or labels.dtype not in LABEL_KINDS:
        return False
    n = mask.numel()
    return rois.shape[-1] == 7 and gt.shape[-1] >= 7 and src.shape[-1] == gt.shape[-1] and cls.numel() == n and reg.numel() == n * 7 \
        and rois.numel() == n * 7 and gt.numel() == n * gt.shape[-1] and src.numel() == gt.numel() and labels.numel() == n


def _workspace(nbytes, device, stream):
    """per (device, stream): allocated through _lib.workspace, its 256-byte head zeroed ONCE -- every call leaves it zero"""
    from ._lib import workspace
    key = (device.index, stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = workspace(max(nbytes, 1 << 16), device)
        ws[:256].zero_()
    return ws


class RoiLossFunction(torch.autograd.Function):
    """(rcnn_loss, [cls, reg, corner, reg + corner, rcnn_loss]) of the ROI head in one launch each way"""

    @staticmethod
    def forward(ctx, rcnn_cls, rcnn_reg, rois, gt, src, mask, labels, with_corner, cls_weight, reg_weight, corner_weight):
        from ._lib import check, lib, ptr, stream_ptr
        L = lib()
        N = int(mask.numel())
        dev = rcnn_cls.device
        cls_c, reg_c = rcnn_cls.contiguous(), rcnn_reg.contiguous()
        rois, gt, src, mask, labels = rois.contiguous(), gt.contiguous(), src.contiguous(), mask.contiguous(), labels.contiguous()
        out = torch.empty((5,), dtype=torch.float32, device=dev)         # cls | reg | corner | reg + corner | cls + (reg + corner)
        norms = torch.empty((2,), dtype=torch.float32, device=dev)
        stream = stream_ptr()
        ws_bytes = int(L.btc_roi_loss_ws_bytes(N))
        ws = _workspace(ws_bytes, dev, stream)
        p = (lambda t: ptr(t) if N else None)
        meta = (int(gt.shape[-1]), p(mask), p(labels), LABEL_KINDS[labels.dtype], N, int(bool(with_corner)), float(cls_weight), float(reg_weight),
                float(corner_weight))
        check(L.btc_roi_loss_fwd(p(cls_c), p(reg_c), p(rois), p(gt), p(src), *meta, ptr(out), ptr(norms), ptr(ws), ws_bytes, stream), "btc_roi_loss_fwd")
        ctx.save_for_backward(cls_c, reg_c, rois, gt, src, mask, labels, norms)
        ctx.meta = meta
        # -> (the loss the head returns, made by the kernel; the five scalars for logging).  Two views of one buffer, as AnchorLossFunction's
        parts = out[:5]
        ctx.mark_non_differentiable(parts)
        return out[4], parts

    @staticmethod
    def backward(ctx, grad_total, _grad_parts):
        from ._lib import check, lib, ptr, stream_ptr
        cls_c, reg_c, rois, gt, src, mask, labels, norms = ctx.saved_tensors
        N = ctx.meta[4]
        d_cls, d_reg = torch.empty_like(cls_c), torch.empty_like(reg_c)           # (the kernel writes every element: no fills)
        g = grad_total.reshape(1).to(torch.float32).contiguous()
        p = (lambda t: ptr(t) if N else None)
        check(lib().btc_roi_loss_bwd(p(cls_c), p(reg_c), p(rois), p(gt), p(src), *ctx.meta, ptr(norms), ptr(g), p(d_cls), p(d_reg), stream_ptr()),
              "btc_roi_loss_bwd")
        return d_cls, d_reg, None, None, None, None, None, None, None, None, None


def roi_loss(ret, weights, with_corner=True):
    """ret: the head's forward_ret_dict -- rcnn_cls (N) or (N, 1), rcnn_reg (N, 7), rois (B, R, 7), gt_of_rois and gt_of_rois_src (B, R, >= 7),
    reg_valid_mask (B, R) int64, rcnn_cls_labels (B, R) float32 or int64, N = B * R; weights: LOSS_WEIGHTS with rcnn_cls_weight,
    rcnn_reg_weight and (with_corner) rcnn_corner_weight -> (total, parts (5) = cls, reg, corner, reg + corner, total).  Only enqueues on
    the current stream."""
    if not usable(ret):
        raise ValueError("roi_loss: float32 predictions, rois and boxes, an int64 mask and float32 or int64 labels on the GPU only "
                         "(there is no CPU fallback in here)")
    cw = float(weights["rcnn_corner_weight"]) if with_corner else 0.0
    return RoiLossFunction.apply(*(ret[k] for k in KEYS), bool(with_corner), float(weights["rcnn_cls_weight"]), float(weights["rcnn_reg_weight"]), cw)
