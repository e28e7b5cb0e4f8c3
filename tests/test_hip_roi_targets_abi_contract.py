"""The buffer contract of btc_roi_targets (include/btcdet_hip_roi_targets.h), as the other contract files hold their entry points to it:
every output is a Guarded buffer (poisoned payload between two guard bands) with spare entries past its extent, the workspace is all
zero as the header asks and is followed by garbage (both patterns) the call must not touch, the call runs on a side stream.  Afterwards
the stated extent is fully overwritten and equals the restatement of tests/roi_targets_ref.py, nothing past it and no guard is touched,
the counters are zero again and the inputs hold the bits they held.  NaN in rois that are never sampled changes nothing but their own
max_overlaps entries.  Refused arguments return -1, write nothing and enqueue nothing."""
import ctypes

import numpy as np
import pytest
import torch

import abi_contract as ac
import roi_targets_ref as rr

pytestmark = pytest.mark.gpu
SPARE = 3
TAIL = 1024
OUTS = (("rois", 7, "float32"), ("gt_of_rois", 8, "float32"), ("gt_of_rois_src", 8, "float32"), ("gt_iou_of_rois", 1, "float32"), ("roi_scores", 1, "float32"),
        ("roi_labels", 1, "int64"), ("reg_valid_mask", 1, "int64"), ("rcnn_cls_labels", 1, None), ("max_overlaps", 1, "float32"), ("gt_assignment", 1, "int64"),
        ("sampled_inds", 1, "int64"))


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _buffers(case):
    B, N = case["rois"].shape[:2]
    R = int(case["cfg"].ROI_PER_IMAGE)
    cls_dt = "float32" if case["cfg"].CLS_SCORE_TYPE == "roi_iou" else "int64"
    rows = lambda k: B * (N if k in ("max_overlaps", "gt_assignment") else R)
    return {k: ac.Guarded((rows(k) + SPARE, w), dt or cls_dt) for k, w, dt in OUTS}, rows


def _call(case, t, outs, ws, sampled_in=None, **kw):
    from btcdet_amd.roi_targets_device import config_block
    B, N = case["rois"].shape[:2]
    blk = config_block(case["cfg"])
    args = [t["rois"].data_ptr(), t["roi_scores"].data_ptr(), t["roi_labels"].data_ptr(), t["gt_boxes"].data_ptr(),
            None if sampled_in is not None else t["uniforms"].data_ptr(), sampled_in.data_ptr() if sampled_in is not None else None, B, N,
            case["gt_boxes"].shape[1], ctypes.byref(blk)] + [outs[k].ptr for k, _, _ in OUTS] + [ws.ptr, L().btc_roi_targets_ws_bytes(B, N)]
    ac.call("btc_roi_targets", *args)


def _extent(outs, rows, case):
    B, N = case["rois"].shape[:2]
    R = int(case["cfg"].ROI_PER_IMAGE)
    got = {}
    for k, w, _ in OUTS:
        n = rows(k)
        gd = outs[k]
        assert not bool(gd.poison_mask()[:n].any()), "%s: an element of the stated extent was left unwritten" % k
        assert bool(gd.poison_mask()[n:].all()) and gd.guards_intact(), "%s: written past its extent" % k
        a = gd.tensor[:n].cpu().numpy()
        got[k] = a.reshape((B, N) if k in ("max_overlaps", "gt_assignment") else ((B, R, w) if w > 1 else (B, R)))
    return got


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("name", ["n63", "n128_quota", "n257_quota_plus_1", "r200_n63"])
def test_roi_targets_buffer_contract(name, garbage):
    from btcdet_amd.iou3d_nms import _pairwise
    case = rr.make_case(rr.CASES[rr.CASE_IDS.index(name)])
    B, N = case["rois"].shape[:2]
    t = {k: _dev(case[k]) for k in ("rois", "roi_scores", "roi_labels", "gt_boxes", "uniforms")}
    before = {k: v.clone() for k, v in t.items()}
    ws_bytes = L().btc_roi_targets_ws_bytes(B, N)
    assert ws_bytes == 256
    ws = ac.Workspace(ws_bytes + TAIL, zero_head=ws_bytes, garbage=garbage)          # a dirty tail behind the stated size
    outs, rows = _buffers(case)
    _call(case, t, outs, ws)
    assert ws.head_zero() and ws.guards_intact() and bool((ws.tensor[ws_bytes:] == garbage).all())
    got = _extent(outs, rows, case)
    for k, v in before.items():
        assert _same_bits(t[k], v), "input %s was written" % k
    bev = np.stack([_pairwise(t["rois"][b], t["gt_boxes"][b][:, :7].contiguous(), 0).cpu().numpy() for b in range(B)])
    rr.check_outputs(got, rr.restate(case, bev, np.float32), rr.restate(case, bev, np.float64), name)
    # the same workspace again without clearing, the draw handed over: nothing is sampled, everything else as before
    outs2, _ = _buffers(case)
    _call(case, t, outs2, ws, sampled_in=_dev(got["sampled_inds"]))
    assert ws.head_zero() and bool((ws.tensor[ws_bytes:] == garbage).all())
    got2 = _extent(outs2, rows, case)
    for k in got:
        assert rr.same_bits(got[k], got2[k]), k


def test_nan_in_unsampled_rois_changes_nothing_else():
    case = rr.make_case(rr.CASES[rr.CASE_IDS.index("n257_quota_plus_1")])
    B, N = case["rois"].shape[:2]
    t = {k: _dev(case[k]) for k in ("rois", "roi_scores", "roi_labels", "gt_boxes", "uniforms")}
    ws = ac.Workspace(256, zero_head=256)
    outs, rows = _buffers(case)
    _call(case, t, outs, ws)
    clean = _extent(outs, rows, case)
    unsampled = np.setdiff1d(np.arange(N), clean["sampled_inds"][0])
    assert unsampled.size > 20
    hit = unsampled[::3]
    rois = case["rois"].copy()
    rois[0, hit] = np.nan
    scores = case["roi_scores"].copy()
    scores[0, hit] = np.nan
    t["rois"], t["roi_scores"] = _dev(rois), _dev(scores)
    outs2, _ = _buffers(case)
    _call(case, t, outs2, ws, sampled_in=_dev(clean["sampled_inds"]))      # (the draw handed over: a NaN overlap would resize the candidate sets)
    dirty = _extent(outs2, rows, case)
    assert ws.head_zero()
    keep = np.ones(N, bool)
    keep[hit] = False
    for k in clean:
        if k in ("max_overlaps", "gt_assignment"):
            assert rr.same_bits(clean[k][0, keep], dirty[k][0, keep]), k
        else:
            assert rr.same_bits(clean[k], dirty[k]), k
    # a NaN roi belongs to no candidate set: whatever its entry holds, it is neither foreground nor background
    c = rr.consts(case["cfg"])
    ov = dirty["max_overlaps"][0, hit]
    assert not (ov >= c.fg_thresh).any() and not (ov < c.reg_fg).any()


def test_roi_targets_refusals_write_nothing():
    from btcdet_amd._lib import stream_ptr
    from btcdet_amd.roi_targets_device import config_block
    case = rr.make_case(rr.CASES[rr.CASE_IDS.index("n63")])
    B, N = case["rois"].shape[:2]
    G = case["gt_boxes"].shape[1]
    t = {k: _dev(case[k]) for k in ("rois", "roi_scores", "roi_labels", "gt_boxes", "uniforms")}
    sel = torch.zeros((B, 128), dtype=torch.int64, device="cuda")
    ws = ac.Workspace(256 + TAIL, zero_head=256)
    outs, _ = _buffers(case)
    names = ["in_rois", "in_scores", "in_labels", "gts", "uniforms", "sampled_in", "B", "N", "G", "cfg"] + [k for k, _, _ in OUTS] + ["ws", "ws_bytes"]
    cases = [dict(B=0), dict(B=-1), dict(N=0), dict(N=1025), dict(G=0), dict(R=0), dict(R=1025), dict(fg_quota=-1), dict(fg_quota=129), dict(score_type=2),
             dict(score_type=-1), dict(cfg=None), dict(in_rois=None), dict(in_scores=None), dict(in_labels=None), dict(gts=None), dict(uniforms=None),
             dict(sampled_in=sel.data_ptr()), dict(ws=None), dict(ws_bytes=255), dict(ws_bytes=0), dict(B=2 ** 19, N=1024), dict(G=2 ** 28)]
    cases += [{k: None} for k, _, _ in OUTS]
    for kw in cases:
        blk = config_block(case["cfg"])
        kw = dict(kw)
        for f in ("R", "fg_quota", "score_type"):
            if f in kw:
                setattr(blk, f, kw.pop(f))
        good = dict(zip(names, [t["rois"].data_ptr(), t["roi_scores"].data_ptr(), t["roi_labels"].data_ptr(), t["gt_boxes"].data_ptr(), t["uniforms"].data_ptr(),
                                None, B, N, G, ctypes.byref(blk)] + [outs[k].ptr for k, _, _ in OUTS] + [ws.ptr, 256]))
        assert L().btc_roi_targets(*dict(good, **kw).values(), stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    for k, gd in outs.items():
        assert bool(gd.poison_mask().all()) and gd.guards_intact(), k
    assert ws.guards_intact() and ws.head_zero() and bool((ws.tensor[256:] == 0xA5).all()), "a refused call touched the workspace"
