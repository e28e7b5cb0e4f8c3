"""KITTI evaluation without a GPU: the numpy restatement (tests/kitti_eval_ref.py) equals what the reference's own eval.py produced
(tests/golden/kitti_eval.npz, tests/golden/gen_kitti_eval_golden.py), the margins function does its job, the host half of
btcdet_amd/kitti_eval.py (clean_data vectorised, get_thresholds, the curves, the annotation builder) equals the restatement, and the
argument checks of the new entry points return before any launch."""
import ctypes

import numpy as np
import pytest

import kitti_eval_ref as ref

golden, case = ref.load_golden, ref.cached_case


@pytest.mark.parametrize("name", sorted(ref.GOLDEN_CASES))
def test_restatement_equals_the_reference(name):
    z, meta = golden()
    gt, dt, classes, cov, per, (res, ret, _) = case(name)
    assert meta[name]["frames"] == len(gt) and meta[name]["n_dt"] == sum(len(a["name"]) for a in dt)
    for m in range(3):
        for k in ("recall", "real_recall", "precision"):
            assert np.array_equal(per[m][k], z["%s/m%d/%s" % (name, m, k)], equal_nan=True), (m, k)
        np.testing.assert_allclose(per[m]["orientation"], z["%s/m%d/orientation" % (name, m)], rtol=1e-9, atol=0, equal_nan=True)
    assert res == meta[name]["result"]
    assert set(ret) == set(meta[name]["ret_dict"])
    for k, v in meta[name]["ret_dict"].items():
        np.testing.assert_allclose(ret[k], v, rtol=1e-9, atol=0, equal_nan=True, err_msg=k)


def test_golden_cases_cover_what_they_claim():
    z, meta = golden()
    assert meta["no_aos"]["compute_aos"] is False and "aos" not in meta["no_aos"]["result"]
    assert meta["three"]["compute_aos"] is True and "Car_aos/moderate_R40" in meta["three"]["ret_dict"]
    assert meta["no_gt"]["ret_dict"]["Cyclist_3d/moderate_R40"] == 0.0        # a class without ground truth: AP 0, no NaN
    assert not z["no_gt/m2/precision"][1].any()
    gt, dt = case("three")[:2]
    names = set(np.concatenate([a["name"] for a in gt]))
    assert {"Van", "Person_sitting", "DontCare"} <= names
    assert z["three/m2/precision"].max() > 0.5      # the curves are not empty
    gt, dt = case("tied")[:2]
    s = np.concatenate([a["score"] for a in dt])
    assert len(np.unique(s)) <= 9 < len(s)


def test_margins_reject_a_planted_near_threshold_pair():
    gt, dt = ref.make_case(seed=5, n_frames=1, sizes=[(1, 1)], gt_names=["Car"], det_names=["Car"])
    g, d = gt[0], dt[0]
    g["rotation_y"][:] = 0.3
    for k in ("location", "dimensions", "rotation_y"):
        d[k] = g[k].copy()
    d["bbox"] = g["bbox"].copy()
    assert ref.margins(gt, dt)["level"] >= ref.MARGIN["level"]          # IoU 1 everywhere: far from every level
    d["dimensions"] = g["dimensions"] * np.array([0.70005, 1.0, 1.0])    # same centre, same angle, shorter: BEV IoU = 0.70005
    (bbox, bev, d3), _ = ref.frame_overlaps(g, d)
    assert abs(bev[0, 0] - 0.70005) < 1e-12
    w = ref.margins(gt, dt)
    assert w["level"] < ref.MARGIN["level"] and not ref.margins_ok(w)
    # two candidates of one ground truth closer than 2e-4
    gt2, dt2 = ref.make_case(seed=6, n_frames=1, sizes=[(1, 2)], gt_names=["Car"], det_names=["Car"])
    g, d = gt2[0], dt2[0]
    for k in ("location", "dimensions"):
        d[k] = np.stack([g[k][0], g[k][0]])
    d["rotation_y"] = np.array([g["rotation_y"][0]] * 2)
    d["dimensions"] = d["dimensions"] * np.array([[0.9, 1, 1], [0.9001, 1, 1]])
    w = ref.margins(gt2, dt2)
    assert w["gap"] < ref.MARGIN["gap"] and not ref.margins_ok(w)
    # a height on a limit
    gt3, dt3 = ref.make_case(seed=7, n_frames=1, sizes=[(1, 1)], gt_names=["Car"], det_names=["Car"])
    gt3[0]["bbox"][0, 3] = gt3[0]["bbox"][0, 1] + 40.0
    assert ref.margins(gt3, dt3)["limit"] < ref.MARGIN["limit"]


def test_clip_area_is_exact_geometry():
    a = [1.0, 2.0, 4.0, 2.0, 0.7]
    assert abs(ref.clip_area(a, a) - 8.0) < 1e-12                                   # identical
    assert abs(ref.clip_area(a, [1.0, 2.0, 2.0, 1.0, 0.7]) - 2.0) < 1e-12           # nested, equal angles
    assert abs(ref.clip_area(a, [1.0, 2.0, 1.0, 1.0, 0.2]) - 1.0) < 1e-12           # nested, another angle
    assert ref.clip_area([0, 0, 2, 2, 0.0], [2, 0, 2, 2, 0.0]) == 0.0               # a shared edge
    assert abs(ref.clip_area([0, 0, 2, 2, 0.0], [1, 1, 2, 2, 0.0]) - 1.0) < 1e-12   # axis-aligned
    assert abs(ref.clip_area([0, 0, 2, 2, 0.0], [0, 0, 2, 2, np.pi / 4]) - (8 * np.sqrt(2) - 8)) < 1e-12    # a regular octagon
    assert ref.clip_area([0, 0, 2, 2, 0.3], [10, 0, 2, 2, 0.1]) == 0.0


# ------------------------------------------------------------------------------------------------------------------ the product's host half
def test_vectorised_clean_data_equals_the_per_box_rules():
    from btcdet_amd import kitti_eval as ke
    gt, dt = case("three")[:2]
    ds = ke.Dataset(gt, dt, device="cpu")
    for diffs in ([0, 1, 2], ref.COVERAGE_RATES):
        classes = [0, 1, 2, 3]
        ign_gt, ign_dt, n_valid = ke.clean_data(ds, classes, diffs)
        for ci, c in enumerate(classes):
            for di, d in enumerate(diffs):
                exp = [ref.clean_data(g, t, c, d) for g, t in zip(gt, dt)]
                assert np.array_equal(ign_gt[ci * len(diffs) + di], np.concatenate([e[0] for e in exp]))
                assert np.array_equal(ign_dt[ci * len(diffs) + di], np.concatenate([e[1] for e in exp]))
                assert n_valid[ci, di] == sum(e[2] for e in exp)
    dc = np.concatenate([g["bbox"][g["name"] == "DontCare"] for g in gt])
    assert np.array_equal(ds.dc_boxes, dc) and ds.h_frames[-1, 2] == len(dc)


def test_get_thresholds_and_curves_equal_the_loops():
    from btcdet_amd import kitti_eval as ke
    rng = np.random.default_rng(3)
    for n, num_gt, tied in ((0, 5, False), (1, 1, False), (7, 9, False), (30, 31, True), (200, 230, False), (500, 501, True), (41, 41, False)):
        s = rng.integers(1, 10, n) / 10.0 if tied else rng.uniform(0, 1, n)
        a, b = ke.get_thresholds(s.copy(), num_gt), ref.get_thresholds(s.copy(), num_gt)
        assert len(a) == len(b) <= 41 and np.array_equal(np.array(a), np.array(b))
    for n in (0, 1, 17, 41):
        pr = np.zeros((n, 4))
        pr[:, :3] = rng.integers(0, 50, (n, 3))
        pr[:, 3] = rng.uniform(0, 1, n) * pr[:, 0]
        if n > 2:
            pr[2, :2] = 0      # tp + fp == 0: the reference divides 0 by 0 there
        counts = np.zeros((1, 41, 3), dtype=np.int32)
        counts[0, :n] = pr[:, :3]
        sim = np.zeros((1, 41))
        sim[0, :n] = pr[:, 3]
        got = ke._curves(counts, sim, np.array([n]), True)
        for g, e in zip(got, ref.curves(pr, True)):
            assert np.array_equal(g[0], e, equal_nan=True)


def test_annotation_builder_equals_the_reference():
    from btcdet_amd import kitti_eval as ke
    z, meta = golden()
    for seed in (1, 2):
        calib, boxes = ref.make_calib(seed), ref.make_lidar_boxes(seed, 40)
        keep = boxes.copy()
        cam = ke.boxes3d_lidar_to_kitti_camera(boxes, calib)
        img = ke.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=meta["builder/%d" % seed]["image_shape"])
        assert np.array_equal(boxes, keep)
        np.testing.assert_allclose(cam, z["builder/%d/camera" % seed], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(img, z["builder/%d/image" % seed], rtol=1e-5, atol=1e-5)
        shape = meta["builder/%d" % seed]["image_shape"]
        assert img[:, [0, 2]].max() <= shape[1] - 1 and img[:, [1, 3]].max() <= shape[0] - 1 and img.min() >= 0
        assert (img[:, 0] == 0).any() or (img[:, 2] == shape[1] - 1).any()      # the clip is exercised


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_return_before_any_launch():
    """1025 detections or ground truths in a frame, a negative count, a table that does not start at 0, a bad metric range, no class and
    a short workspace are BTC_EINVAL with a message; the (never dereferenced) pointers are not device memory"""
    from btcdet_amd import _lib
    L = _lib.lib()
    p = 0x1000

    def table(rows):
        a = np.ascontiguousarray(np.array(rows, dtype=np.int32))
        return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def overlaps(rows):
        a, hp = table(rows)
        return L.btc_kitti_overlaps(p, p, p, p, p, hp, len(rows) - 1, p, p, None)

    def match_tp(rows, m0=0, M=3, C=1, D=3, K=2):
        a, hp = table(rows)
        return L.btc_kitti_match_tp(p, p, p, p, p, p, p, hp, len(rows) - 1, m0, M, C, D, K, p, p, None)

    def stats(rows, ws_bytes, aos=1, C=1):
        a, hp = table(rows)
        return L.btc_kitti_match_stats(p, p, p, p, p, p, p, p, p, p, p, hp, len(rows) - 1, 0, 3, C, 3, 2, aos, p, p, p, ws_bytes, None)

    ok = [[0, 0, 0], [5, 7, 1]]
    assert overlaps([[0, 0, 0], [5, 1025, 0]]) == -1 and b"1025 detections" in L.btc_last_error()
    assert overlaps([[0, 0, 0], [1025, 5, 0]]) == -1 and b"1025 ground truths" in L.btc_last_error()
    assert overlaps([[0, 0, 0], [5, 7, 1], [4, 9, 1]]) == -1 and b"negative count" in L.btc_last_error()
    assert overlaps([[1, 0, 0], [5, 7, 1]]) == -1 and b"start at 0" in L.btc_last_error()
    assert L.btc_kitti_overlaps(p, p, p, p, p, None, 1, p, p, None) == -1
    assert L.btc_kitti_overlaps(p, p, p, p, p, table(ok)[1], -1, p, p, None) == -1
    assert match_tp([[0, 0, 0], [5, 1025, 0]]) == -1 and b"1025 detections" in L.btc_last_error()
    assert match_tp(ok, m0=1, M=3) == -1 and b"metrics" in L.btc_last_error()
    assert match_tp(ok, M=0) == -1
    assert match_tp(ok, C=0) == -1 and b"0 classes" in L.btc_last_error()
    assert stats(ok, 8) == -1 and b"workspace too small" in L.btc_last_error()
    assert stats([[0, 0, 0], [5, 1025, 0]], 1 << 20) == -1 and b"1025 detections" in L.btc_last_error()
    assert L.btc_kitti_match_stats_ws_bytes(10, 3, 3, 2, 1) >= 10 * 18 * 41 * 8
    assert L.btc_kitti_match_stats_ws_bytes(10, 3, 3, 2, 0) == 256


def test_multi_classes_nms_stays_unimplemented():
    import types
    from btcdet_amd.predictor import BtcPredictor
    cfg = types.SimpleNamespace(NMS_CONFIG=types.SimpleNamespace(MULTI_CLASSES_NMS=True))
    model = types.SimpleNamespace(heads="full", eval=lambda: model)
    with pytest.raises(NotImplementedError):
        BtcPredictor(model, post_cfg=cfg, num_class=3)
