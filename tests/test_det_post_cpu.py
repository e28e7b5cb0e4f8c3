"""CPU-side checks of the detections feature (no GPU is touched): the numpy restatement the GPU tests rely on equals the golden vectors
the reference's own Detector3DTemplate.post_processing wrote; the POST_PROCESSING yaml blocks hold the reference's values; both new
entry points refuse bad arguments before any launch; MULTI_CLASSES_NMS and stacked inputs raise.

Tolerances.  Every decision -- which boxes, their order, labels, counts, every recall counter, the presence of `iou` -- is compared
exactly: the generator asserts margins of 1e-5 (scores) and 1e-4 / 2e-4 (IoUs) around every threshold it crosses.  Score VALUES are
compared within 1e-6: the golden scores come from torch's CPU sigmoid, the restatement's from a float64 exp rounded to fp32, a few fp32
ulps (6e-8 each) apart at most.  Raw scores are inputs passed through: exact.  IoU values at rtol 1e-4 / atol 2e-5, the project's IoU
tolerance (the restatement multiplies the same oracle overlaps in numpy instead of torch)."""
import numpy as np
import pytest

import det_post_ref as ref


@pytest.mark.parametrize("name", list(ref.CASES))
def test_restatement_equals_the_golden_file(name):
    g = ref.load_golden()
    bd, num_class = ref.case_inputs(name)
    cfg = ref.case_cfg(name)
    scenes, recall = ref.restate(bd, cfg, num_class)
    assert recall == ref.golden_recall(g, name, cfg)
    for b, sc in enumerate(scenes):
        want = ref.golden_scene(g, name, b)
        assert np.array_equal(sc["selected"], want["selected"]), (name, b)
        assert np.array_equal(sc["labels"], want["labels"]), (name, b)
        if cfg["OUTPUT_RAW_SCORE"]:
            assert np.array_equal(sc["scores"], want["scores"])
        else:
            assert np.allclose(sc["scores"], want["scores"], rtol=0, atol=1e-6)
        assert (sc["iou"] is None) == (want["iou"] is None), (name, b)
        if want["iou"] is not None:
            assert sc["iou"].shape == want["iou"].shape
            assert np.allclose(sc["iou"], want["iou"], rtol=1e-4, atol=2e-5)


def test_golden_file_covers_the_listed_cases():
    """a scene without ground truth counts one; a scene without detections has empty outputs and no iou; truncation truncates"""
    g = ref.load_golden()
    assert int(g["configured_recall"][0]) == 11                      # 5 + 5 boxes and one all-zero row
    assert len(g["no_detections_1_selected"]) == 0 and int(g["no_detections_1_has_iou"]) == 0
    assert all(len(g["truncate_%d_selected" % b]) == 5 for b in range(3))
    assert any(int(g["no_rois_%d_has_iou" % b]) for b in range(3)) and not any(int(g["configured_%d_has_iou" % b]) for b in range(3))
    assert set(np.concatenate([g["class_labels_%d_labels" % b] for b in range(3)]).tolist()) <= {1, 2, 3}
    assert len(set(np.concatenate([g["three_class_%d_labels" % b] for b in range(3)]).tolist())) == 3
    assert all(len(g["pre_max_%d_selected" % b]) <= 12 for b in range(3))
    assert all(len(g["large_%d_selected" % b]) > 0 and int(g["large_%d_selected" % b].max()) > 1024 for b in range(3))


def test_yaml_blocks_equal_the_reference_values():
    import os
    from btcdet_amd.config import load_cfg
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for f in ("btcdet_kitti_car.yaml", "btcdet_waymo_synth.yaml"):
        pp = load_cfg(os.path.join(root, "btcdet_amd", "cfgs", f)).MODEL.POST_PROCESSING
        assert pp == ref.BASE_CFG, f
        assert pp.RECALL_THRESH_LIST == [0.3, 0.5, 0.7] and pp.SCORE_THRESH == 0.6 and pp.OUTPUT_RAW_SCORE is False
        n = pp.NMS_CONFIG
        assert (n.NMS_TYPE, n.NMS_THRESH, n.NMS_PRE_MAXSIZE, n.NMS_POST_MAXSIZE, n.MULTI_CLASSES_NMS) == ("nms_gpu", 0.1, 4096, 500, False)


P = 0x1000      # a non-null address nobody reads: every call below returns from its argument checks


def _select(L, n=100, num_class=1, stride=7, pre=4096, post=500, cls=P, boxes=P, keep=P, num=P, best=P, ws=P, ws_bytes=1 << 30, batch=2):
    return L.btc_det_select_nms(cls, boxes, batch, n, num_class, stride, 0, 0.6, 0.1, 1, pre, post, keep, num, best, ws, ws_bytes, None)


def _finish(L, n=100, num_class=1, stride=7, post=500, T=3, cls=P, boxes=P, keep=P, num=P, best=P, gt=P, counters=P, out=P, thr=True, batch=2):
    import ctypes
    h = (ctypes.c_float * 16)(*([0.5] * 16))
    return L.btc_det_finish(cls, boxes, batch, n, num_class, stride, 0, 0, keep, num, best, None, post, gt, 12, 8, None, 0, 0,
                            ctypes.cast(h, ctypes.POINTER(ctypes.c_float)) if thr else None, T, out, out, out, out, counters, None)


def test_select_nms_argument_checks_return_before_any_launch():
    from btcdet_amd import _lib
    L = _lib.lib()
    assert _select(L, n=1025) == -1 and b"1024" in L.btc_last_error()
    assert _select(L, num_class=0) == -1 and b"num_class" in L.btc_last_error()
    assert _select(L, post=4097) == -1 and b"post_max" in L.btc_last_error()
    assert _select(L, post=0) == -1
    assert _select(L, pre=0) == -1
    assert _select(L, stride=6) == -1 and b"box_stride" in L.btc_last_error()
    assert _select(L, batch=-1) == -1
    for kw in ("cls", "boxes", "keep", "num", "best", "ws"):
        assert _select(L, **{kw: None}) == -1 and b"missing pointer" in L.btc_last_error(), kw
    assert _select(L, ws_bytes=16) == -1 and b"workspace too small" in L.btc_last_error()
    assert L.btc_det_select_nms_ws_bytes(2, 100) >= 2 * 4 + 2 * 100 * 2 * 8
    assert _select(L, batch=0) == 0          # nothing to do, nothing launched


def test_finish_argument_checks_return_before_any_launch():
    from btcdet_amd import _lib
    L = _lib.lib()
    assert _finish(L, T=9) == -1 and b"recall thresholds" in L.btc_last_error()
    assert _finish(L, num_class=0) == -1 and b"num_class" in L.btc_last_error()
    assert _finish(L, post=4097) == -1 and b"post_max" in L.btc_last_error()
    assert _finish(L, stride=6) == -1
    for kw in ("cls", "boxes", "keep", "num", "best", "out", "counters"):
        assert _finish(L, **{kw: None}) == -1 and b"missing pointer" in L.btc_last_error(), kw
    assert _finish(L, thr=False) == -1 and b"missing pointer" in L.btc_last_error()
    assert _finish(L, batch=0) == 0


class _Cfg(dict):
    __getattr__ = dict.__getitem__


def _cfg(**nms):
    c = _Cfg(ref.BASE_CFG)
    c["NMS_CONFIG"] = _Cfg(dict(ref.BASE_CFG["NMS_CONFIG"], **nms))
    return c


def test_unsupported_inputs_raise():
    import torch
    from btcdet_amd import post_processing as pp
    bd = {"batch_size": 2, "batch_cls_preds": torch.zeros(2, 10, 1), "batch_box_preds": torch.zeros(2, 10, 7), "cls_preds_normalized": False}
    with pytest.raises(NotImplementedError):
        pp.detect(bd, _cfg(MULTI_CLASSES_NMS=True), 1)
    with pytest.raises(NotImplementedError):
        pp.post_processing(bd, _cfg(MULTI_CLASSES_NMS=True), 1)
    stacked = {"batch_size": 2, "batch_cls_preds": torch.zeros(20, 1), "batch_box_preds": torch.zeros(20, 7), "cls_preds_normalized": False,
               "batch_index": torch.zeros(20)}
    with pytest.raises(NotImplementedError):
        pp.post_processing(stacked, _cfg(), 1)
    with pytest.raises(NotImplementedError):
        pp.detect(bd, _cfg(NMS_TYPE="nms_cpu"), 1)


def test_predictor_refuses_a_model_without_heads_and_multi_class_nms():
    from btcdet_amd.predictor import BtcPredictor

    class M(object):
        heads = None

        def eval(self):
            return self

    with pytest.raises(ValueError):
        BtcPredictor(M())
    m = M()
    m.heads = "full"
    with pytest.raises(NotImplementedError):
        BtcPredictor(m, post_cfg=_cfg(MULTI_CLASSES_NMS=True), num_class=1)
