"""Detections on the GPU (btcdet_amd/post_processing.py over csrc/det_post.hip; btcdet_amd/predictor.py).

Against tests/golden/det_post.npz -- the reference's own Detector3DTemplate.post_processing -- and, on seeded cases the golden file does
not hold, against the numpy restatement tests/test_det_post_cpu.py pins to that file.  Every decision is compared EXACTLY: kept indices
and their order, labels, counts, every recall counter, the presence of `iou`; boxes are gathered, so bit-equal; raw scores exact.  Both
the generator and det_post_ref.seeded_case keep the inputs 1e-5 (scores) / 1e-4 (NMS IoU) / 2e-4 (recall IoU) away from every
threshold, more than twice the project's IoU tolerance.  Values: sigmoid scores within 1e-6 absolute (a few fp32 ulps between the
device expf and the CPU's), `iou` at rtol 1e-4 / atol 2e-5 (tests/test_hip_iou3d_nms.py's tolerance)."""
import numpy as np
import pytest
import torch

import det_post_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


class Cfg(dict):
    __getattr__ = dict.__getitem__


def to_cfg(d):
    return Cfg({k: (to_cfg(v) if isinstance(v, dict) else v) for k, v in d.items()})


def to_device(bd):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in bd.items()}


def check_against(bd, cfg, pred_dicts, recall, scenes, want_recall, what):
    assert recall == want_recall, (what, recall, want_recall)
    assert len(pred_dicts) == len(scenes)
    for b, (p, w) in enumerate(zip(pred_dicts, scenes)):
        boxes, scores, labels = p["pred_boxes"].cpu().numpy(), p["pred_scores"].cpu().numpy(), p["pred_labels"].cpu().numpy()
        print(what, "scene", b, "kept", len(scores), "expected", len(w["selected"]),
              "max |score diff|", float(np.abs(scores - w["scores"]).max()) if len(scores) == len(w["scores"]) and len(scores) else None)
        assert boxes.shape == (len(w["selected"]), bd["batch_box_preds"].shape[2]) and scores.shape == w["scores"].shape and labels.shape == w["labels"].shape
        assert p["pred_labels"].dtype == torch.int64
        assert np.array_equal(boxes, bd["batch_box_preds"][b][w["selected"]]), (what, b, "boxes: kept indices or their order differ")
        assert np.array_equal(labels, w["labels"]), (what, b)
        if cfg["OUTPUT_RAW_SCORE"]:
            assert np.array_equal(scores, w["scores"]), (what, b)
        else:
            assert np.allclose(scores, w["scores"], rtol=0, atol=1e-6), (what, b)
        assert (p["iou"] is None) == (w["iou"] is None), (what, b, "iou presence")
        if w["iou"] is not None:
            assert isinstance(p["iou"], np.ndarray) and p["iou"].shape == w["iou"].shape
            assert np.allclose(p["iou"], w["iou"], rtol=1e-4, atol=2e-5), (what, b, float(np.abs(p["iou"] - w["iou"]).max()))


def run_paths(bd, cfg, num_class):
    """-> {path: (pred_dicts, recall_dict)}: the fused kernels (n <= 1024) and the path behind the anchor head"""
    from btcdet_amd import post_processing as pp
    n = bd["batch_box_preds"].shape[1]
    dbd = to_device(bd)
    before = {k: v.clone() for k, v in dbd.items() if torch.is_tensor(v)}
    out = {}
    for path in (["fused", "large"] if n <= pp.FUSED_MAX_BOXES else ["large"]):
        out[path] = pp.post_processing(dbd, to_cfg(cfg), num_class, path=path)
    out["default"] = pp.post_processing(dbd, to_cfg(cfg), num_class)
    for k, v in before.items():
        assert torch.equal(dbd[k], v), "input %s was written" % k
    return out


@pytest.mark.parametrize("name", list(ref.CASES))
def test_against_the_reference_golden_vectors(name):
    g = ref.load_golden()
    bd, num_class = ref.case_inputs(name)
    cfg = ref.case_cfg(name)
    scenes = [ref.golden_scene(g, name, b) for b in range(bd["batch_size"])]
    for path, (pred_dicts, recall) in run_paths(bd, cfg, num_class).items():
        check_against(bd, cfg, pred_dicts, recall, scenes, ref.golden_recall(g, name, cfg), "%s/%s" % (name, path))


SEEDED = {
    "n1": dict(seed=1, B=2, n=1, logits=(2.0, 2.0)),
    "n63": dict(seed=2, B=3, n=63),
    "n64-three-class-normalized": dict(seed=8, B=2, n=64, num_class=3, normalized=True),
    "n65-axis-aligned": dict(seed=9, B=5, n=65, nms={"NMS_TYPE": "nms_normal_gpu"}),
    "n100-b8-rois-labels": dict(seed=3, B=8, n=100, rois=True, labels=True),
    "n100-all-kept-rois": dict(seed=15, B=2, n=100, rois=True, logits=(0.5, 3.5), nms={"NMS_THRESH": 0.999}),   # kept = n: `iou` over the input boxes
    "n257-zero-boxes-ties": dict(seed=6, B=2, n=257, zero_boxes=40, dup_scores=60),
    "n257-raw-score": dict(seed=10, B=2, n=257, cfg={"OUTPUT_RAW_SCORE": True}, dup_scores=20),
    "n1000-all-below": dict(seed=7, B=2, n=1000, logits=(-6.0, -1.0)),
    "n1000-pre-max": dict(seed=11, B=3, n=1000, nms={"NMS_PRE_MAXSIZE": 200}),
    "n1000-post-max": dict(seed=12, B=3, n=1000, nms={"NMS_POST_MAXSIZE": 37}),
    "n1024": dict(seed=4, B=2, n=1024, rois=True),
    "n1024-all-above": dict(seed=5, B=2, n=1024, logits=(0.5, 3.5)),
    "n1024-all-above-post-max-64": dict(seed=13, B=3, n=1024, logits=(0.5, 3.5), nms={"NMS_POST_MAXSIZE": 64}),
    "n3000-large-only": dict(seed=14, B=2, n=3000, logits=(-14.0, 1.6)),
}


@pytest.mark.parametrize("name", list(SEEDED))
def test_fused_path_large_path_and_restatement_agree(name):
    bd, cfg, (scenes, want_recall) = ref.seeded_case(**SEEDED[name])
    kw = SEEDED[name]
    if "pre-max" in name:
        assert all(int((ref.sigmoid32(bd["batch_cls_preds"][b]).max(-1) >= 0.6).sum()) > 200 for b in range(kw["B"]))
    if "post-max" in name:
        assert all(len(s["selected"]) == cfg["NMS_CONFIG"]["NMS_POST_MAXSIZE"] for s in scenes)
    if "all-below" in name:
        assert all(len(s["selected"]) == 0 for s in scenes)
    if "all-kept" in name:
        assert all(len(s["selected"]) == kw["n"] and s["iou"] is not None for s in scenes[:-1])
    for path, (pred_dicts, recall) in run_paths(bd, cfg, kw.get("num_class", 1)).items():
        check_against(bd, cfg, pred_dicts, recall, scenes, want_recall, "%s/%s" % (name, path))


def test_detect_outputs_are_padded_with_zeros_and_resident():
    from btcdet_amd import post_processing as pp
    bd, cfg, (scenes, _) = ref.seeded_case(seed=3, B=8, n=100, rois=True, labels=True)
    for path in ("fused", "large"):
        det = pp.detect(to_device(bd), to_cfg(cfg), 1, path=path)
        K = cfg["NMS_CONFIG"]["NMS_POST_MAXSIZE"]
        assert det.boxes.shape == (8, K, 7) and det.scores.shape == (8, K) and det.labels.shape == (8, K) and det.iou.shape == (8, K)
        assert all(t.is_cuda for t in (det.boxes, det.scores, det.labels, det.num, det.iou, det.recall))
        assert det.num.dtype == torch.int32 and det.labels.dtype == torch.int64 and det.recall.dtype == torch.int64
        num = det.num.cpu().numpy()
        assert num.tolist() == [len(s["selected"]) for s in scenes]
        for b in range(8):
            assert not bool(det.boxes[b, num[b]:].any()) and not bool(det.scores[b, num[b]:].any()) and not bool(det.labels[b, num[b]:].any())


def test_recall_counters_accumulate_over_two_calls():
    from btcdet_amd import post_processing as pp
    a, cfg, (_, ra) = ref.seeded_case(seed=3, B=8, n=100, rois=True, labels=True)
    b, _, (_, rb) = ref.seeded_case(seed=21, B=3, n=63, rois=True)
    for path in ("fused", "large"):
        rec = pp.new_recall(cfg["RECALL_THRESH_LIST"], DEV)
        d1 = pp.detect(to_device(a), to_cfg(cfg), 1, recall=rec, path=path)
        assert d1.recall is rec
        assert pp.recall_dict_from(rec.cpu().numpy(), cfg["RECALL_THRESH_LIST"]) == ra
        pp.detect(to_device(b), to_cfg(cfg), 1, recall=rec, path=path)
        got = pp.recall_dict_from(rec.cpu().numpy(), cfg["RECALL_THRESH_LIST"])
        assert got == {k: ra[k] + rb[k] for k in ra}, (path, got)


def test_no_ground_truth_means_no_record():
    from btcdet_amd import post_processing as pp
    bd, cfg, (scenes, _) = ref.seeded_case(seed=2, B=3, n=63)
    bd = {k: v for k, v in bd.items() if k != "gt_boxes"}
    pred_dicts, recall = pp.post_processing(to_device(bd), to_cfg(cfg), 1)
    assert recall == {} and all(p["iou"] is None for p in pred_dicts)
    assert [len(p["pred_scores"]) for p in pred_dicts] == [len(s["selected"]) for s in scenes]


def test_detect_reads_nothing_back():
    """detect() under torch's sync debug mode "error" raises nothing on either path; an .item() inside that mode does raise on this build
    (shown first -- otherwise the mode proves nothing and the test skips)"""
    from btcdet_amd import post_processing as pp
    small, cfg, _ = ref.seeded_case(seed=3, B=8, n=100, rois=True, labels=True)
    big, cfg_big, _ = ref.seeded_case(seed=14, B=2, n=3000, logits=(-14.0, 1.6))
    dsmall, dbig = to_device(small), to_device(big)
    pp.detect(dsmall, to_cfg(cfg), 1)          # (first calls: library load, allocator growth)
    pp.detect(dbig, to_cfg(cfg_big), 1)
    probe = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.sum().item()
            raised = False
        except RuntimeError:
            raised = True
        if not raised:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag .item() on this build: the mode cannot show the absence of a read-back")
        d1 = pp.detect(dsmall, to_cfg(cfg), 1, path="fused")
        d2 = pp.detect(dsmall, to_cfg(cfg), 1, path="large")
        d3 = pp.detect(dbig, to_cfg(cfg_big), 1)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    assert torch.equal(d1.num, d2.num) and torch.equal(d1.boxes, d2.boxes) and int(d3.num.sum()) > 0


# ---------------------------------------------------------------------------------------------------------------- BtcPredictor
def _model_and_batches():
    import bench
    from btcdet_amd.btc_path import BtcHotPath
    from btcdet_amd.config import load_cfg
    torch.manual_seed(0)
    np.random.seed(0)
    model = BtcHotPath(load_cfg(), device=torch.device(DEV), heads="full").to(DEV)
    batches = bench.build_batches(2, 3, torch.device(DEV))
    model.train()
    with torch.no_grad():
        for b in batches:        # running statistics other than their initial values
            model(model.prepare(b))
    return model.eval(), batches


def test_predictor_on_two_synthetic_batches(monkeypatch):
    """predict() equals post_processing() applied to the forward's own batch_dict, the model's forward outputs are bit-identical with and
    without the predictor around it, the record accumulates over the batches, and no parameter or buffer moves.  (Deterministic library
    algorithms are requested as in tests/test_hip_eval_fold.py: torch's Conv1d of the ROI head otherwise moves bits from run to run.)"""
    from btcdet_amd import post_processing as pp
    from btcdet_amd.predictor import BtcPredictor
    model, batches = _model_and_batches()
    cfg = model.cfg.MODEL.POST_PROCESSING
    # an untrained head scores everything near 0.5: a threshold the synthetic scores straddle, so that detections exist
    low = to_cfg(dict(ref.BASE_CFG, SCORE_THRESH=0.0, NMS_CONFIG=dict(ref.BASE_CFG["NMS_CONFIG"])))
    state = {k: v.clone() for k, v in model.state_dict().items()}
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    det = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        for post_cfg in (cfg, low):
            pred = BtcPredictor(model, post_cfg=post_cfg)
            total = None
            for batch in batches:
                with torch.no_grad():
                    _, _, bd = model(model.prepare(batch, is_train=False))
                fwd = pred.forward(batch)
                for k in ("batch_cls_preds", "batch_box_preds", "rois", "roi_labels"):
                    assert torch.equal(fwd[k], bd[k]), k
                want_dicts, want_recall = pp.post_processing(bd, post_cfg, pred.num_class)
                got_dicts, got_recall = pred.predict(batch)
                assert got_recall == want_recall and set(got_recall) == {"gt", "roi_0.3", "rcnn_0.3", "roi_0.5", "rcnn_0.5", "roi_0.7", "rcnn_0.7"}
                assert len(got_dicts) == bd["batch_size"]
                for g_, w_ in zip(got_dicts, want_dicts):
                    for k in ("pred_boxes", "pred_scores", "pred_labels"):
                        assert torch.equal(g_[k], w_[k]), k
                    assert (g_["iou"] is None) == (w_["iou"] is None) and (g_["iou"] is None or np.array_equal(g_["iou"], w_["iou"]))
                if post_cfg is low:
                    assert sum(len(d["pred_scores"]) for d in got_dicts) > 0
                d = pred(batch)                     # the resident form: same numbers, the record added once more
                assert d.num.cpu().tolist() == [len(x["pred_scores"]) for x in got_dicts]
                total = want_recall if total is None else {k: total[k] + want_recall[k] for k in total}
            assert pred.recall_summary() == {k: 2 * v for k, v in total.items()}
    finally:
        torch.use_deterministic_algorithms(det[0], warn_only=det[1])
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k
