"""The buffer contract of btc_kitti_overlaps / btc_kitti_match_tp / btc_kitti_match_stats (include/btcdet_hip_infer.h), as
tests/test_hip_det_post_abi_contract.py holds the detection entry points to it: every output is a Guarded buffer (poisoned payload between
two guard bands), the workspace is garbage.  After the calls every output is fully overwritten, the guards are intact, the inputs hold the
bits they held, and the same calls on the current stream give the same bits.  Refused arguments write nothing.

(abi_contract.POISON has no float64 entry: a float64 output is allocated as int64 of the same shape -- the same 8-byte slots, poisoned
with the int64 pattern -- and read through a float64 view.)"""
import ctypes

import numpy as np
import pytest
import torch

import abi_contract as ac
import kitti_eval_ref as ref

pytestmark = pytest.mark.gpu


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _on(stream, fn, *args):
    torch.cuda.current_stream().synchronize()
    rc = fn(*args, stream.cuda_stream)
    stream.synchronize()
    assert rc == 0, "rc %d: %s" % (rc, L().btc_last_error().decode("utf-8", "replace"))


def _g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _hp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


# name -> (make_case arguments, classes): tiny, empty frames in between, a state wider than one mask word, the limit
CONTRACT = {
    "tiny": (dict(seed=51, n_frames=1, sizes=[(2, 3)]), ["Car"]),
    "empty_between": (dict(seed=52, n_frames=9, max_gt=5, max_dt=7, empty_every=2), ["Car", "Pedestrian", "Cyclist"]),
    "wide": (dict(seed=34, n_frames=2, sizes=[(70, 140), (3, 2)], gt_names=["Car", "Car", "Pedestrian", "DontCare"]), ["Car", "Pedestrian"]),
    "limit": (dict(seed=35, n_frames=1, sizes=[(4, 1024)], gt_names=["Car", "Car", "Pedestrian", "DontCare"], pad_real=0.0), ["Car"]),
}


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("name", sorted(CONTRACT))
def test_kitti_eval_buffer_contract(name, garbage):
    from btcdet_amd import kitti_eval as ke
    from btcdet_amd._lib import check, ptr, stream_ptr
    kw, classes = CONTRACT[name]
    gt, dt = ref.make_case(**kw)
    ds = ke.Dataset(gt, dt)
    ci = ref.classes_to_int(classes)
    C, D, K, M = len(ci), 3, 2, 3
    combos, cdk = M * C * D * K, C * D * K
    ign_gt, ign_dt, n_valid = ke.clean_data(ds, ci, [0, 1, 2])
    d = ds.dev()
    g_ig, g_id, g_mo = _g(ign_gt), _g(ign_dt), _g(ref.official_min_overlaps(ci))
    inputs = [d["gt"], d["dt"], d["dc"], d["frames"], d["pairs"], g_ig, g_id, g_mo]
    before = [t.clone() for t in inputs]
    hf = _hp(ds.h_frames)
    ws_bytes = L().btc_kitti_match_stats_ws_bytes(ds.F, C, D, K, 1)
    s = torch.cuda.Stream()

    def run(ov, ov_dc, tp_det, tp_count, counts, sim, ws_ptr, side):
        def call(fn, *a):
            if side:
                _on(s, fn, *a)
            else:
                check(fn(*a, stream_ptr()), "kitti eval")
                torch.cuda.synchronize()
        call(L().btc_kitti_overlaps, ptr(d["gt"]), ptr(d["dt"]), ptr(d["dc"]), ptr(d["frames"]), ptr(d["pairs"]), hf, ds.F, ov, ov_dc)
        call(L().btc_kitti_match_tp, ov, ptr(d["dt"]), ptr(g_ig), ptr(g_id), ptr(g_mo), ptr(d["frames"]), ptr(d["pairs"]), hf, ds.F, 0, M, C, D, K,
             tp_det, tp_count)
        return lambda thr, nthr: call(L().btc_kitti_match_stats, ov, ov_dc, ptr(d["gt"]), ptr(d["dt"]), ptr(g_ig), ptr(g_id), ptr(g_mo), ptr(thr),
                                      ptr(nthr), ptr(d["frames"]), ptr(d["pairs"]), hf, ds.F, 0, M, C, D, K, 1, counts, sim, ws_ptr, ws_bytes)

    def thresholds(tp_det):
        h = tp_det.cpu().numpy()
        thr, nthr = np.zeros((combos, 41)), np.zeros((combos,), np.int32)
        for co in range(combos):
            t = ke.get_thresholds(ds.dt_rows[h[co][h[co] >= 0], 12], int(n_valid[(co // (K * D)) % C, (co // K) % D]))
            nthr[co], thr[co, :len(t)] = len(t), t
        return _g(thr), _g(nthr)

    ws = ac.Workspace(ws_bytes, garbage=garbage)
    outs = {"ov": ac.Guarded((3, ds.P), "int64"), "ov_dc": ac.Guarded((ds.PD,), "int64"), "tp_det": ac.Guarded((combos, ds.NG), "int32"),
            "tp_count": ac.Guarded((combos,), "int32"), "counts": ac.Guarded((combos, 41, 3), "int32"), "sim": ac.Guarded((cdk, 41), "int64")}
    stats = run(outs["ov"].ptr, outs["ov_dc"].ptr, outs["tp_det"].ptr, outs["tp_count"].ptr, outs["counts"].ptr, outs["sim"].ptr, ws.ptr, True)
    thr, nthr = thresholds(outs["tp_det"].tensor)
    inputs += [thr, nthr]
    before += [thr.clone(), nthr.clone()]
    stats(thr, nthr)
    for k, g in outs.items():
        assert not bool(g.poison_mask().any()), "%s: %d of %d elements left as poison" % (k, int(g.poison_mask().sum()), g.tensor.numel())
        assert g.guards_intact(), k
    assert ws.guards_intact()
    ov = outs["ov"].tensor.view(torch.float64)
    assert bool(((ov >= 0) & (ov <= 1 + 1e-9)).all()) and bool(torch.isfinite(outs["sim"].tensor.view(torch.float64)).all())
    tp_det = outs["tp_det"].tensor
    assert bool(((tp_det >= -1) & (tp_det < max(ds.ND, 1))).all())
    assert torch.equal((tp_det >= 0).sum(1).to(torch.int32), outs["tp_count"].tensor)
    assert bool((outs["counts"].tensor[:, :, [0, 2]] >= 0).all())
    for t, b in zip(inputs, before):
        assert torch.equal(t, b), "an input was written"
    # the same calls on the current stream (an ordinary workspace, no guards) give the same bits
    dev = d["gt"].device
    again = {"ov": torch.empty((3, ds.P), dtype=torch.int64, device=dev), "ov_dc": torch.empty((ds.PD,), dtype=torch.int64, device=dev),
             "tp_det": torch.empty((combos, ds.NG), dtype=torch.int32, device=dev), "tp_count": torch.empty((combos,), dtype=torch.int32, device=dev),
             "counts": torch.empty((combos, 41, 3), dtype=torch.int32, device=dev), "sim": torch.empty((cdk, 41), dtype=torch.int64, device=dev)}
    w2 = torch.empty((max(ws_bytes, 256),), dtype=torch.uint8, device=dev)
    run(ptr(again["ov"]), ptr(again["ov_dc"]), ptr(again["tp_det"]), ptr(again["tp_count"]), ptr(again["counts"]), ptr(again["sim"]), ptr(w2), False)(thr, nthr)
    for k in outs:
        assert torch.equal(again[k], outs[k].tensor), k


def test_nothing_is_written_when_the_arguments_are_refused():
    from btcdet_amd import kitti_eval as ke
    from btcdet_amd._lib import ptr, stream_ptr
    gt, dt = ref.make_case(seed=52, n_frames=4, max_gt=5, max_dt=7)
    ds = ke.Dataset(gt, dt)
    d = ds.dev()
    C, D, K, M = 1, 3, 2, 3
    combos = M * C * D * K
    ign_gt, ign_dt, _ = ke.clean_data(ds, [0], [0, 1, 2])
    g_ig, g_id, g_mo = _g(ign_gt), _g(ign_dt), _g(ref.official_min_overlaps([0]))
    thr, nthr = torch.zeros((combos, 41), dtype=torch.float64, device="cuda"), torch.zeros((combos,), dtype=torch.int32, device="cuda")
    ws_bytes = L().btc_kitti_match_stats_ws_bytes(ds.F, C, D, K, 1)
    ws = ac.Workspace(ws_bytes)
    ov, ov_dc = ac.Guarded((3, ds.P), "int64"), ac.Guarded((max(ds.PD, 1),), "int64")
    tp_det, tp_count = ac.Guarded((combos, ds.NG), "int32"), ac.Guarded((combos,), "int32")
    counts, sim = ac.Guarded((combos, 41, 3), "int32"), ac.Guarded((C * D * K, 41), "int64")
    over = ds.h_frames.copy()
    over[1:, 1] += 1025 - (over[1, 1] - over[0, 1])        # 1025 detections in the first frame
    over_gt = ds.h_frames.copy()
    over_gt[1:, 0] += 1025 - (over_gt[1, 0] - over_gt[0, 0])
    neg = ds.h_frames.copy()
    neg[2, 1] = neg[1, 1] - 1                              # a negative count
    for h in (over, over_gt, neg):
        h = np.ascontiguousarray(h)
        assert L().btc_kitti_overlaps(ptr(d["gt"]), ptr(d["dt"]), ptr(d["dc"]), ptr(d["frames"]), ptr(d["pairs"]), _hp(h), ds.F, ov.ptr, ov_dc.ptr,
                                      stream_ptr()) == -1
        assert L().btc_kitti_match_tp(ov.ptr, ptr(d["dt"]), ptr(g_ig), ptr(g_id), ptr(g_mo), ptr(d["frames"]), ptr(d["pairs"]), _hp(h), ds.F, 0, M, C, D, K,
                                      tp_det.ptr, tp_count.ptr, stream_ptr()) == -1
    hf = _hp(ds.h_frames)
    assert L().btc_kitti_overlaps(ptr(d["gt"]), ptr(d["dt"]), ptr(d["dc"]), ptr(d["frames"]), ptr(d["pairs"]), hf, -1, ov.ptr, ov_dc.ptr, stream_ptr()) == -1
    for kw in (dict(m0=2, M=2), dict(C=0), dict(K=0), dict(D=-1)):
        assert L().btc_kitti_match_tp(ov.ptr, ptr(d["dt"]), ptr(g_ig), ptr(g_id), ptr(g_mo), ptr(d["frames"]), ptr(d["pairs"]), hf, ds.F, kw.get("m0", 0),
                                      kw.get("M", M), kw.get("C", C), kw.get("D", D), kw.get("K", K), tp_det.ptr, tp_count.ptr, stream_ptr()) == -1, kw
    for kw in (dict(ws_bytes=8), dict(h=np.ascontiguousarray(over)), dict(M=4), dict(nthr=None)):
        rc = L().btc_kitti_match_stats(ov.ptr, ov_dc.ptr, ptr(d["gt"]), ptr(d["dt"]), ptr(g_ig), ptr(g_id), ptr(g_mo), ptr(thr),
                                       ptr(kw.get("nthr", nthr)), ptr(d["frames"]), ptr(d["pairs"]), _hp(kw["h"]) if "h" in kw else hf, ds.F, 0,
                                       kw.get("M", M), C, D, K, 1, counts.ptr, sim.ptr, ws.ptr, kw.get("ws_bytes", ws_bytes), stream_ptr())
        assert rc == -1, kw
    torch.cuda.synchronize()
    for g in (ov, ov_dc, tp_det, tp_count, counts, sim):
        assert bool(g.poison_mask().all()) and g.guards_intact()
    assert ws.guards_intact() and bool((ws.tensor == 0xA5).all())
