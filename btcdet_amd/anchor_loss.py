"""The anchor head's loss on the GPU (csrc/anchor_loss.hip, include/btcdet_hip_anchor_loss.h): forward one launch, backward one launch.

    total, parts = anchor_loss(cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets, flat_anchors, weights, dir_offset)
    # total: rpn_loss, differentiable with respect to the three prediction tensors; parts (4): cls, loc, dir, total -- not differentiable

What is replaced: dense_head.AnchorHeadSingle.get_loss in the reference's formulation -- a one-hot tensor over (B, A, C + 1), the anchors
repeated per scene, two cats for the heading products, several dozen elementwise launches and an autograd twin for each -- by
btc_anchor_loss_fwd and btc_anchor_loss_bwd.  The inputs are exactly what DeviceTargetAssigner leaves on the device (int32 labels,
float32 targets, its flat_anchors); nothing is converted, read back or synchronised, and the sums are deterministic.

Dropped quirk of the reference: with one class it overwrites every positive label with 1 IN PLACE; here the labels keep their bits and
a positive label simply counts as class 1.  Kept: no code weights (built and never applied), a NaN regression target contributes
nothing, the per-scene normaliser max(#positives, 1).

Opt-in: dense_head.AnchorHeadSingle.get_loss uses this module when LOSS_CONFIG.DEVICE is set and `unsupported_reason` is None.  A call
whose tensors are not on the GPU or not float32 (labels: int32) takes the torch route for that call -- `usable` decides; the CPU golden
vectors of the head depend on it.  There is no CPU fallback in here: anchor_loss() on CPU tensors raises."""
import torch

from .anchor_targets import MAX_CLASSES, _get

MAX_BINS = 16                       # BTC_ANCHOR_LOSS_MAX_BINS of include/btcdet_hip_anchor_loss.h
THREADS, MAX_TILES = 256, 512       # BTC_ANCHOR_LOSS_THREADS, BTC_ANCHOR_LOSS_MAX_TILES

_WS = {}


def unsupported_reason(model_cfg, box_coder, num_class=None):
    """None when btc_anchor_loss_* computes what the torch route of get_loss would, else a sentence naming the option that bars it"""
    if _get(model_cfg, "USE_MULTIHEAD", False):
        return "USE_MULTIHEAD is not computed on the device"
    if getattr(box_coder, "encode_angle_by_sincos", False):
        return "encode_angle_by_sincos is not computed on the device"
    if getattr(box_coder, "code_size", 7) != 7:
        return "a box code size of %d (not 7) is not computed on the device" % box_coder.code_size
    if num_class is not None and not 1 <= num_class < MAX_CLASSES:
        return "%d classes do not fit the kernel's limit (1 <= C < %d)" % (num_class, MAX_CLASSES)
    if _get(model_cfg, "USE_DIRECTION_CLASSIFIER", None) is not None and not 1 <= int(_get(model_cfg, "NUM_DIR_BINS", 0)) <= MAX_BINS:
        return "NUM_DIR_BINS %s does not fit the kernel's limit (1 <= bins <= %d)" % (_get(model_cfg, "NUM_DIR_BINS", None), MAX_BINS)
    return None


def usable(cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets):
    """this call's tensors are what the kernels take: on the GPU, float32 (labels int32)"""
    floats = [cls_preds, box_preds, box_reg_targets] + ([dir_cls_preds] if dir_cls_preds is not None else [])
    return all(t.is_cuda and t.dtype == torch.float32 for t in floats) and box_cls_labels.is_cuda and box_cls_labels.dtype == torch.int32


def _workspace(nbytes, device, stream):
    """per (device, stream): allocated through _lib.workspace, its 256-byte head zeroed ONCE -- every call leaves it zero"""
    from ._lib import workspace
    key = (device.index, stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = workspace(max(nbytes, 1 << 16), device)
        ws[:256].zero_()
    return ws


class AnchorLossFunction(torch.autograd.Function):
    """(rpn_loss, [cls, loc, dir, rpn_loss]) of the anchor head in one launch each way"""

    @staticmethod
    def forward(ctx, cls_preds, box_preds, dir_cls_preds, labels, targets, anchors, cls_weight, loc_weight, dir_weight, dir_offset):
        from ._lib import check, lib, ptr, stream_ptr
        L = lib()
        B, A, C = (int(v) for v in cls_preds.shape)
        bins = int(dir_cls_preds.shape[2]) if dir_cls_preds is not None else 0
        dev = cls_preds.device
        cls_c, box_c = cls_preds.contiguous(), box_preds.contiguous()
        dir_c = dir_cls_preds.contiguous() if dir_cls_preds is not None else None
        labels, targets, anchors = labels.contiguous(), targets.contiguous(), anchors.contiguous()
        out = torch.empty((4,), dtype=torch.float32, device=dev)       # cls | loc | dir | cls + (loc + dir)
        norms = torch.empty((B,), dtype=torch.float32, device=dev)
        stream = stream_ptr()
        ws_bytes = int(L.btc_anchor_loss_ws_bytes(B, A))
        ws = _workspace(ws_bytes, dev, stream)
        p = (lambda t: ptr(t) if A else None)
        scal = (float(cls_weight), float(loc_weight), float(dir_weight), float(dir_offset))
        check(L.btc_anchor_loss_fwd(p(cls_c), p(box_c), p(dir_c), p(labels), p(targets), p(anchors), B, A, C, bins, *scal, ptr(out), ptr(norms),
                                    ptr(ws), ws_bytes, stream), "btc_anchor_loss_fwd")
        ctx.save_for_backward(cls_c, box_c, dir_c, labels, targets, anchors, norms)
        ctx.meta = (B, A, C, bins) + scal
        # -> (the loss the head returns, made by the kernel; the four scalars for logging).  Two views of one buffer, as OccLossFunction's
        parts = out[:4]
        ctx.mark_non_differentiable(parts)
        return out[3], parts

    @staticmethod
    def backward(ctx, grad_total, _grad_parts):
        from ._lib import check, lib, ptr, stream_ptr
        cls_c, box_c, dir_c, labels, targets, anchors, norms = ctx.saved_tensors
        B, A, C, bins = ctx.meta[:4]
        d_cls, d_box = torch.empty_like(cls_c), torch.empty_like(box_c)          # (the kernel writes every element: no fills)
        d_dir = torch.empty_like(dir_c) if dir_c is not None else None
        g = grad_total.reshape(1).to(torch.float32).contiguous()
        p = (lambda t: ptr(t) if A else None)
        check(lib().btc_anchor_loss_bwd(p(cls_c), p(box_c), p(dir_c), p(labels), p(targets), p(anchors), B, A, C, bins, *ctx.meta[4:], ptr(norms), ptr(g),
                                        p(d_cls), p(d_box), p(d_dir), stream_ptr()), "btc_anchor_loss_bwd")
        return d_cls, d_box, d_dir, None, None, None, None, None, None, None


def anchor_loss(cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets, anchors, weights, dir_offset=0.0):
    """cls_preds (B, A, C), box_preds (B, A, 7), dir_cls_preds (B, A, bins) or None, box_cls_labels (B, A) int32, box_reg_targets (B, A, 7),
    anchors (A, 7) in DeviceTargetAssigner.flat_anchors order; weights: LOSS_WEIGHTS with cls_weight, loc_weight and (with a direction
    classifier) dir_weight -> (total, parts (4) = cls, loc, dir, total).  Only enqueues on the current stream."""
    if not usable(cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets):
        raise ValueError("anchor_loss: float32 predictions and targets and int32 labels on the GPU only (there is no CPU fallback in here)")
    B, A = int(cls_preds.shape[0]), int(cls_preds.shape[1])
    if cls_preds.dim() != 3 or tuple(box_preds.shape) != (B, A, 7) or tuple(box_cls_labels.shape) != (B, A) or tuple(box_reg_targets.shape) != (B, A, 7) \
            or tuple(anchors.shape) != (A, 7) or (dir_cls_preds is not None and tuple(dir_cls_preds.shape[:2]) != (B, A)):
        raise ValueError("anchor_loss: shapes cls %r box %r dir %r labels %r targets %r anchors %r" % tuple(
            None if t is None else tuple(t.shape) for t in (cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets, anchors)))
    if anchors.dtype != torch.float32 or anchors.device != cls_preds.device:
        raise ValueError("anchor_loss: anchors must be float32 on %s" % cls_preds.device)
    dw = float(weights["dir_weight"]) if dir_cls_preds is not None else 0.0
    return AnchorLossFunction.apply(cls_preds, box_preds, dir_cls_preds, box_cls_labels, box_reg_targets, anchors, float(weights["cls_weight"]),
                                    float(weights["loc_weight"]), dw, float(dir_offset))
