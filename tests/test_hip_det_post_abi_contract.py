"""The buffer contract of btc_det_select_nms / btc_det_finish (include/btcdet_hip_infer.h), as tests/test_hip_infer_abi_contract.py holds
btc_conv_bn_eval_fwd to it: every output is a Guarded buffer (poisoned payload between two guard bands), the workspace is garbage.  After a
call every output is fully overwritten -- padding included --, the guards are intact, the inputs hold the bits they held, and the same
call on the current stream gives the same bits.  Refused arguments write nothing."""
import ctypes

import numpy as np
import pytest
import torch

import abi_contract as ac
import det_post_ref as ref

pytestmark = pytest.mark.gpu

THR = (ctypes.c_float * 3)(0.3, 0.5, 0.7)
THR_P = ctypes.cast(THR, ctypes.POINTER(ctypes.c_float))


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _call_on_stream(stream, fn, *args):
    torch.cuda.current_stream().synchronize()
    rc = fn(*args, stream.cuda_stream)
    stream.synchronize()
    assert rc == 0, "rc %d: %s" % (rc, L().btc_last_error().decode("utf-8", "replace"))


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# (n, B, classes, post_max, rois, labels, rotated): one row block, several, the limit; truncating post_max; every optional input
CONTRACT = [(1, 1, 1, 8, False, False, 1), (64, 3, 1, 500, True, True, 1), (100, 8, 3, 500, True, False, 1), (257, 2, 1, 20, False, True, 0),
            (1024, 2, 1, 4096, True, False, 1)]


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("n,B,C,post,rois,labels,rotated", CONTRACT)
def test_det_post_buffer_contract(n, B, C, post, rois, labels, rotated, garbage):
    from btcdet_amd._lib import check, ptr, stream_ptr
    bd, cfg, _ = ref.seeded_case(seed=100 + n, B=B, n=n, num_class=C, rois=rois, labels=labels, logits=(2.0, 2.0) if n == 1 else (-4.0, 4.0),
                                 nms={"NMS_POST_MAXSIZE": post, "NMS_TYPE": "nms_gpu" if rotated else "nms_normal_gpu"})
    cls, boxes, gt = _g(bd["batch_cls_preds"]), _g(bd["batch_box_preds"]), _g(bd["gt_boxes"])
    roi = _g(bd["rois"]) if rois else None
    lab = _g(bd["roi_labels"]) if labels else None
    inputs = [t for t in (cls, boxes, gt, roi, lab) if t is not None]
    before = [t.clone() for t in inputs]
    G = gt.shape[1]
    s = torch.cuda.Stream()

    def run(keep, num, best, pb, ps, pl, pi, counters, ws_ptr, ws_bytes, on_stream):
        a1 = (ptr(cls), ptr(boxes), B, n, C, 7, 0, 0.6, 0.1, rotated, 4096, post, keep, num, best, ws_ptr, ws_bytes)
        a2 = (ptr(cls), ptr(boxes), B, n, C, 7, 0, 0, keep, num, best, ptr(lab), post, ptr(gt), G, 8, ptr(roi), n if rois else 0, 7 if rois else 0, THR_P, 3,
              pb, ps, pl, pi, counters)
        if on_stream:
            _call_on_stream(s, L().btc_det_select_nms, *a1)
            _call_on_stream(s, L().btc_det_finish, *a2)
        else:
            check(L().btc_det_select_nms(*a1, stream_ptr()), "btc_det_select_nms")
            check(L().btc_det_finish(*a2, stream_ptr()), "btc_det_finish")
            torch.cuda.synchronize()

    ws_bytes = L().btc_det_select_nms_ws_bytes(B, n)
    ws = ac.Workspace(ws_bytes, garbage=garbage)
    outs = {"keep": ac.Guarded((B, post), "int64"), "num": ac.Guarded((B,), "int32"), "best": ac.Guarded((B, n), "int32"),
            "boxes": ac.Guarded((B, post, 7), "float32"), "scores": ac.Guarded((B, post), "float32"), "labels": ac.Guarded((B, post), "int64"),
            "iou": ac.Guarded((B, post), "float32")}
    counters = ac.Guarded((7,), "int64", fill=0)        # ADDED TO: starts at zero, not poison
    run(outs["keep"].ptr, outs["num"].ptr, outs["best"].ptr, outs["boxes"].ptr, outs["scores"].ptr, outs["labels"].ptr, outs["iou"].ptr,
        counters.ptr, ws.ptr, ws_bytes, True)
    for k, g in outs.items():
        assert not bool(g.poison_mask().any()), "%s: %d of %d elements left as poison" % (k, int(g.poison_mask().sum()), g.tensor.numel())
        assert g.guards_intact(), k
    assert counters.guards_intact() and ws.guards_intact()
    num = outs["num"].tensor.cpu().numpy()
    assert ((num >= 0) & (num <= min(post, n))).all()
    keep = outs["keep"].tensor.cpu().numpy()
    for b in range(B):
        assert (keep[b, num[b]:] == -1).all() and ((keep[b, :num[b]] >= 0) & (keep[b, :num[b]] < n)).all()
        assert not bool(outs["boxes"].tensor[b, num[b]:].any()) and not bool(outs["scores"].tensor[b, num[b]:].any())
    assert bool(torch.isfinite(outs["boxes"].tensor).all()) and bool(torch.isfinite(outs["iou"].tensor).all())
    for t, b in zip(inputs, before):
        assert torch.equal(t, b), "an input was written"
    # the same calls on the current stream (an ordinary workspace, no guards) give the same bits
    dev = cls.device
    again = {"keep": torch.empty((B, post), dtype=torch.int64, device=dev), "num": torch.empty((B,), dtype=torch.int32, device=dev),
             "best": torch.empty((B, n), dtype=torch.int32, device=dev), "boxes": torch.empty((B, post, 7), device=dev),
             "scores": torch.empty((B, post), device=dev), "labels": torch.empty((B, post), dtype=torch.int64, device=dev),
             "iou": torch.empty((B, post), device=dev)}
    c2 = torch.zeros((7,), dtype=torch.int64, device=dev)
    w2 = torch.empty((max(ws_bytes, 256),), dtype=torch.uint8, device=dev)
    run(ptr(again["keep"]), ptr(again["num"]), ptr(again["best"]), ptr(again["boxes"]), ptr(again["scores"]), ptr(again["labels"]), ptr(again["iou"]),
        ptr(c2), ptr(w2), ws_bytes, False)
    for k in outs:
        assert torch.equal(again[k], outs[k].tensor), k
    assert torch.equal(c2, counters.tensor)


def test_nothing_is_written_when_the_arguments_are_refused():
    from btcdet_amd._lib import ptr, stream_ptr
    B, n, post = 2, 50, 16
    cls, boxes = torch.zeros((B, n, 1), device="cuda"), torch.zeros((B, n, 7), device="cuda")
    ws = ac.Workspace(L().btc_det_select_nms_ws_bytes(B, n))
    keep, num, best = ac.Guarded((B, post), "int64"), ac.Guarded((B,), "int32"), ac.Guarded((B, n), "int32")
    pb, ps, pl, pi = ac.Guarded((B, post, 7), "float32"), ac.Guarded((B, post), "float32"), ac.Guarded((B, post), "int64"), ac.Guarded((B, post), "float32")
    counters = ac.Guarded((7,), "int64")
    for kw in (dict(n=1025), dict(C=0), dict(post=4097), dict(pre=0), dict(ws_bytes=8)):
        rc = L().btc_det_select_nms(ptr(cls), ptr(boxes), B, kw.get("n", n), kw.get("C", 1), 7, 0, 0.6, 0.1, 1, kw.get("pre", 4096), kw.get("post", post),
                                    keep.ptr, num.ptr, best.ptr, ws.ptr, kw.get("ws_bytes", ws.ws_bytes), stream_ptr())
        assert rc == -1, kw
    for kw in (dict(T=9), dict(C=0), dict(post=4097), dict(stride=3)):
        rc = L().btc_det_finish(ptr(cls), ptr(boxes), B, n, kw.get("C", 1), kw.get("stride", 7), 0, 0, keep.ptr, num.ptr, best.ptr, None,
                                kw.get("post", post), None, 0, 0, None, 0, 0, THR_P, kw.get("T", 3), pb.ptr, ps.ptr, pl.ptr, pi.ptr, counters.ptr, stream_ptr())
        assert rc == -1, kw
    torch.cuda.synchronize()
    for g in (keep, num, best, pb, ps, pl, pi, counters):
        assert bool(g.poison_mask().all()) and g.guards_intact()
    assert ws.guards_intact() and bool((ws.tensor == 0xA5).all())
