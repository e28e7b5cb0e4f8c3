"""KITTI evaluation on the GPU (btcdet_amd/kitti_eval.py, csrc/kitti_eval.hip): the overlaps against the float64 convex clipping at the
project's IoU tolerance, exact agreement of the matching with the reference's own eval.py (tests/golden/kitti_eval.npz) and with the
numpy restatement (tests/kitti_eval_ref.py) on seeded cases the file does not hold, the smallest shapes that can go wrong, bit-equal
repeats, and KittiEvaluator.  The restatement of a case is computed once and shared (kitti_eval_ref.cached_case)."""
import numpy as np
import pytest
import torch

import kitti_eval_ref as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5      # the project's IoU tolerance


def ke():
    from btcdet_amd import kitti_eval
    return kitti_eval


def _anno(names, bbox, loc, dims, ry, score=None):
    n = len(names)
    a = {"name": np.array(names, dtype="<U16"), "truncated": np.zeros(n), "occluded": np.zeros(n), "alpha": np.zeros(n),
         "bbox": np.array(bbox, np.float64).reshape(-1, 4), "location": np.array(loc, np.float64).reshape(-1, 3),
         "dimensions": np.array(dims, np.float64).reshape(-1, 3), "rotation_y": np.array(ry, np.float64), "coverage_rates": np.full(n, 0.5)}
    if score is not None:
        a["score"] = np.array(score, np.float64)
    return a


def test_overlaps_of_the_degenerate_pairs():
    """ground truth 0 against: itself bit for bit, a box nested in it, an equal-angle shifted box, a box sharing an edge, a disjoint
    box, and a box over the same footprint but above it; all three metrics and the DontCare variant"""
    g_loc, g_dim, g_ry = [2.0, 1.6, 20.0], [4.0, 1.5, 2.0], 0.4          # dims (l, h, w); BEV rectangle (x, z, l, w, ry)
    c, s = np.cos(g_ry), np.sin(g_ry)
    along = lambda t: [g_loc[0] + c * t, 1.6, g_loc[2] - s * t]          # t metres along the box's own x axis (rotate_iou's convention)
    gt = _anno(["Car", "DontCare"], [[100, 100, 200, 160], [300, 100, 400, 200]], [g_loc, [-1000] * 3], [g_dim, [-1] * 3], [g_ry, -10])
    dt = _anno(["Car"] * 6,
               [[100, 100, 200, 160], [120, 110, 180, 150], [150, 100, 250, 160], [200, 100, 300, 160], [500, 10, 600, 60], [320, 120, 380, 180]],
               [g_loc, g_loc, along(1.0), along(4.0), [40.0, 1.6, 50.0], [2.0, 1.6 - 1.5, 20.0]],
               [g_dim, [2.0, 0.75, 1.0], g_dim, g_dim, g_dim, g_dim], [g_ry, g_ry + 0.3, g_ry, g_ry, 1.0, g_ry], score=[0.9] * 6)
    ds = ke().Dataset([gt], [dt])
    ov, dc = ds.frame_overlaps(0)
    (e2, eb, e3), edc = ref.frame_overlaps(gt, dt)
    for got, exp in ((ov[0], e2), (ov[1], eb), (ov[2], e3), (dc, edc)):
        np.testing.assert_allclose(got, exp, rtol=RTOL, atol=ATOL)
    col = ov[:, :, 0]
    np.testing.assert_allclose(col[:, 0], 1.0, rtol=1e-12)                                  # identical: IoU 1
    np.testing.assert_allclose(col[1, 1], 2.0 / 8.0, rtol=1e-12)                            # nested: the ratio of the areas
    np.testing.assert_allclose(col[2, 1], (2.0 * 0.75) / (4.0 * 1.5 * 2.0), rtol=1e-12)     # nested in 3-D too (0.75 high on the same floor)
    np.testing.assert_allclose(col[1, 2], 3.0 / 5.0, rtol=1e-12)                            # equal angles, shifted 1 m of 4: 3 / (4 + 4 - 3)
    np.testing.assert_allclose(col[0, 2], 50.0 / 150.0, rtol=1e-12)
    assert abs(col[1, 3]) < 1e-12 and abs(col[2, 3]) < 1e-12 and col[0, 3] == 0.0          # a shared edge: no area
    assert (col[:, 4] == 0.0).all()                                                         # disjoint
    np.testing.assert_allclose(col[1, 5], 1.0, rtol=1e-12)                                  # the same footprint ...
    assert col[2, 5] == 0.0                                                                 # ... on top of it: no common height
    assert (ov[1:, :, 1] == 0.0).all()                                                      # nothing touches the DontCare placeholder box
    np.testing.assert_allclose(dc[5, 0], 1.0, rtol=1e-12)                                   # inside the DontCare region: its own area
    assert dc[0, 0] == 0.0


def test_overlaps_of_a_seeded_case():
    gt, dt = ref.cached_case("three")[:2]
    ds = ke().Dataset(gt, dt)
    worst = 0.0
    for f in range(0, len(gt), 3):
        ov, dc = ds.frame_overlaps(f)
        (e2, eb, e3), edc = ref.frame_overlaps(gt[f], dt[f])
        for got, exp in ((ov[0], e2), (ov[1], eb), (ov[2], e3), (dc, edc)):
            np.testing.assert_allclose(got, exp, rtol=RTOL, atol=ATOL)
            if exp.size:
                worst = max(worst, float(np.abs(got - exp).max()))
    print("largest overlap difference", worst)


def _check_against(per_gpu, per_ref, aos):
    for m in range(3):
        for key, pr in per_ref[m]["counts"].items():
            n = len(pr)
            assert per_gpu[m]["n_thresholds"][key] == n, (m, key)
            assert np.array_equal(per_gpu[m]["counts"][key][:n], pr[:, :3].astype(np.int64)), (m, key)     # tp / fp / fn exact
            assert not per_gpu[m]["counts"][key][n:].any()
        for k in ("recall", "real_recall", "precision"):
            assert np.array_equal(per_gpu[m][k], per_ref[m][k], equal_nan=True), (m, k)
        np.testing.assert_allclose(per_gpu[m]["orientation"], per_ref[m]["orientation"], rtol=1e-9, atol=0, equal_nan=True)
    if not aos:
        assert not per_gpu[0]["orientation"].any()


def _evaluate(gt, dt, classes, cov):
    k = ke()
    ds = k.Dataset(gt, dt)
    ci = ref.classes_to_int(classes)
    return k.evaluate(ds, ci, [0, 1, 2] if cov is None else cov, ref.official_min_overlaps(ci), 0, 3, ds.compute_aos), ds.compute_aos


@pytest.mark.parametrize("name", sorted(ref.GOLDEN_CASES))
def test_exact_agreement_with_the_reference(name):
    z, meta = ref.load_golden()
    gt, dt, classes, cov, per_ref, _ = ref.cached_case(name)
    per, aos = _evaluate(gt, dt, classes, cov)
    assert aos == meta[name]["compute_aos"]
    _check_against(per, per_ref, aos)
    for m in range(3):
        for k in ("recall", "real_recall", "precision"):
            assert np.array_equal(per[m][k], z["%s/m%d/%s" % (name, m, k)], equal_nan=True), (m, k)
        np.testing.assert_allclose(per[m]["orientation"], z["%s/m%d/orientation" % (name, m)], rtol=1e-9, atol=0, equal_nan=True)
    detail = {}
    res, ret, prd = ke().get_official_eval_result(gt, dt, classes, coverage_rates=cov, PR_detail_dict=detail)
    assert res == meta[name]["result"]
    assert set(ret) == set(meta[name]["ret_dict"])
    for k, v in meta[name]["ret_dict"].items():
        np.testing.assert_allclose(ret[k], v, rtol=1e-9, atol=0, equal_nan=True, err_msg=k)
    assert set(detail) == ({"bbox", "bev", "3d", "aos"} if aos else {"bbox", "bev", "3d"})
    assert np.array_equal(detail["3d"], z["%s/m2/precision" % name], equal_nan=True)
    assert set(prd) == {"bev", "3d"} and set(prd["3d"]) == set(classes)
    if name == "three":      # more than 41 true positives and fewer, every list a short one (a full one: SHAPES["full"])
        n = np.concatenate([per[m]["n_thresholds"].reshape(-1) for m in range(3)])
        tp = np.concatenate([per[m]["counts"][..., 0].max(-1).reshape(-1) for m in range(3)])
        assert (tp > 41).any() and ((tp > 0) & (tp < 41)).any() and ((n > 0) & (n < 41)).any()
    # eval_class, one metric at a time, is the same computation
    ci = ref.classes_to_int(classes)
    one = ke().eval_class(gt, dt, ci, [0, 1, 2] if cov is None else cov, 2, ref.official_min_overlaps(ci))
    assert one["precision"].shape == (len(ci), 3, 2, 41) and np.array_equal(one["precision"], per[2]["precision"], equal_nan=True)


# seeded cases the golden file does not hold: name -> (make_case arguments, classes)
SHAPES = {
    "nothing": (dict(seed=41, n_frames=1, sizes=[(0, 0)]), ["Car"]),
    "no_gt": (dict(seed=42, n_frames=1, sizes=[(0, 5)]), ["Car", "Pedestrian"]),
    "no_dt": (dict(seed=43, n_frames=1, sizes=[(5, 0)], gt_names=["Car", "Pedestrian"]), ["Car", "Pedestrian"]),
    "wide": (dict(seed=32, n_frames=1, sizes=[(70, 65)], gt_names=["Car", "Car", "Car", "Van", "DontCare"], det_names=("Car",)), ["Car"]),
    "wider": (dict(seed=34, n_frames=2, sizes=[(70, 140), (3, 2)], gt_names=["Car", "Car", "Pedestrian", "DontCare"]), ["Car", "Pedestrian"]),
    "limit": (dict(seed=35, n_frames=1, sizes=[(4, 1024)], gt_names=["Car", "Car", "Pedestrian", "DontCare"], pad_real=0.0), ["Car", "Pedestrian"]),
    "full": (dict(seed=36, n_frames=25, max_gt=8, gt_names=["Car", "Car", "Pedestrian"], found=1.0), ["Car", "Pedestrian"]),
    "interleaved": (dict(seed=33, n_frames=130, max_gt=4, max_dt=6, empty_every=3), ["Car", "Pedestrian"]),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_smallest_shapes_that_can_go_wrong(name):
    kw, classes = SHAPES[name]
    gt, dt, _, _, per_ref, (res_ref, ret_ref, _) = ref.cached_case("shape/" + name, classes=classes, **kw)
    if name == "limit":
        assert len(dt[0]["name"]) == 1024
    per, aos = _evaluate(gt, dt, classes, None)
    _check_against(per, per_ref, aos)
    if name == "full":       # recall reaches 1: a full list of 41 thresholds, from more than 41 true positives
        n = np.concatenate([per[m]["n_thresholds"].reshape(-1) for m in range(3)])
        assert (n == 41).any() and per[0]["counts"][..., 0].max() > 41
    res, ret, _ = ke().get_official_eval_result(gt, dt, classes)
    assert res == res_ref
    for k, v in ret_ref.items():
        np.testing.assert_allclose(ret[k], v, rtol=1e-9, atol=0, equal_nan=True, err_msg=k)


def test_more_than_1024_boxes_in_a_frame_are_refused():
    from btcdet_amd._lib import BtcHipError
    gt, dt = ref.make_case(seed=35, n_frames=1, sizes=[(4, 1024)], gt_names=["Car", "Car", "Pedestrian", "DontCare"], pad_real=0.0)
    for k in dt[0]:
        dt[0][k] = np.concatenate([dt[0][k], dt[0][k][:1]])
    with pytest.raises(BtcHipError, match="1025 detections"):
        ke().get_official_eval_result(gt, dt, ["Car"])


def test_two_runs_give_identical_bits():
    gt, dt, classes, cov, _, _ = ref.cached_case("three")
    a, _ = _evaluate(gt, dt, classes, cov)
    b, _ = _evaluate(gt, dt, classes, cov)
    for m in range(3):
        for k in ("recall", "real_recall", "precision", "orientation", "counts"):
            assert a[m][k].tobytes() == b[m][k].tobytes(), (m, k)
    assert a[0]["orientation"].any()
    d1, d2 = ke().Dataset(gt, dt), ke().Dataset(gt, dt)
    assert torch.equal(d1.overlaps()[0], d2.overlaps()[0]) and torch.equal(d1.overlaps()[1], d2.overlaps()[1])


def test_zero_frames_are_valid():
    """F = 0: nothing is launched but the memsets; every count, the similarity and every AP are zero"""
    import abi_contract as ac
    from btcdet_amd import _lib
    res, ret, prd = ke().get_official_eval_result([], [], ["Car", "Cyclist"])
    res_ref, ret_ref, _ = ref.get_official_eval_result([], [], ["Car", "Cyclist"])
    assert res == res_ref and ret.keys() == ret_ref.keys() and all(v == 0.0 for v in ret.values())
    L = _lib.lib()
    C, D, K, M = 2, 3, 2, 3
    combos = M * C * D * K
    h = np.zeros((1, 3), dtype=np.int32)
    hp = _lib.i3p(h)
    z32, z64 = torch.zeros((1, 3), dtype=torch.int32, device="cuda"), torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    mo = torch.from_numpy(np.ascontiguousarray(ref.official_min_overlaps([0, 2]))).cuda()
    thr, nthr = torch.zeros((combos, 41), dtype=torch.float64, device="cuda"), torch.zeros((combos,), dtype=torch.int32, device="cuda")
    tp_count, counts, sim = ac.Guarded((combos,), "int32"), ac.Guarded((combos, 41, 3), "int32"), ac.Guarded((C * D * K, 41), "int64")
    ws = ac.Workspace(L.btc_kitti_match_stats_ws_bytes(0, C, D, K, 1))
    p, sp = _lib.ptr, _lib.stream_ptr()
    _lib.check(L.btc_kitti_overlaps(None, None, None, p(z32), p(z64), hp, 0, None, None, sp), "btc_kitti_overlaps")
    _lib.check(L.btc_kitti_match_tp(None, None, None, None, p(mo), p(z32), p(z64), hp, 0, 0, M, C, D, K, None, tp_count.ptr, sp), "btc_kitti_match_tp")
    _lib.check(L.btc_kitti_match_stats(None, None, None, None, None, None, p(mo), p(thr), p(nthr), p(z32), p(z64), hp, 0, 0, M, C, D, K, 1,
                                       counts.ptr, sim.ptr, ws.ptr, ws.ws_bytes, sp), "btc_kitti_match_stats")
    torch.cuda.synchronize()
    for g in (tp_count, counts, sim):
        assert not bool(g.tensor.any()) and g.guards_intact()      # fully overwritten: zeros, not the poison
    assert ws.guards_intact()


def test_evaluator_in_three_batches_equals_one_evaluation():
    """ground truths are built from seeded lidar boxes, detections are those boxes jittered: the AP table is not trivial, so a frame put in
    the wrong place by add() changes it"""
    z, meta = ref.load_golden()
    names = ["Car", "Pedestrian", "Cyclist"]
    k = ke()
    frames, gt = [], []
    for f in range(6):
        seed = 1 + f % 2
        calib, shape = ref.make_calib(seed), meta["builder/%d" % seed]["image_shape"]
        rng = np.random.default_rng([9, f])
        true = ref.make_lidar_boxes(10 + f, 9)
        true[:, 0] = rng.uniform(6, 30, len(true))                      # near enough for an image box above the height limits
        labels = rng.integers(1, 4, len(true))
        g = k.prediction_anno({"pred_boxes": true, "pred_scores": np.ones(len(true), np.float32), "pred_labels": labels}, calib, shape, names)
        g["coverage_rates"] = np.full(len(true), 0.5)
        gt.append(g)
        keep = np.arange(len(true))[:0 if f == 4 else 7]                 # frame 4 has no detection
        boxes = true[keep] + rng.normal(0, 0.03, (len(keep), 7)).astype(np.float32)
        frames.append(({"pred_boxes": torch.from_numpy(boxes), "pred_scores": torch.from_numpy(rng.uniform(0.1, 1, len(keep)).astype(np.float32)),
                        "pred_labels": torch.from_numpy(labels[keep])}, calib, shape))
    ev = k.KittiEvaluator(gt, names)
    for lo, hi in ((0, 2), (2, 3), (3, 6)):
        ev.add(list(range(lo, hi)), [frames[i][0] for i in range(lo, hi)], [frames[i][1] for i in range(lo, hi)], [frames[i][2] for i in range(lo, hi)])
    res, ret, _ = ev.result()
    annos = [k.prediction_anno(p, c, s, names, i) for i, (p, c, s) in enumerate(frames)]
    res1, ret1, _ = k.get_official_eval_result(gt, annos, names)
    assert res == res1 and ret.keys() == ret1.keys() and all(np.array_equal(ret[key], ret1[key], equal_nan=True) for key in ret)
    assert max(ret["%s_3d/moderate_R40" % n] for n in names) > 20.0 and ret["Car_bev/hard_R40"] > 0     # a table worth comparing
    swapped = [annos[1], annos[0]] + annos[2:]
    assert k.get_official_eval_result(gt, swapped, names)[0] != res      # the frame order matters to this table
    assert "aos" in res      # alpha is left zero, not -10: the reference computes AOS then
    a = annos[0]
    assert a["name"].shape == (7,) and set(a["name"]) <= set(names) and not a["alpha"].any() and not a["truncated"].any() and not a["occluded"].any()
    assert annos[4]["bbox"].shape == (0, 4) and annos[4]["frame_id"] == 4
    # the builder's camera and image boxes against the reference's two box_utils functions
    for seed in (1, 2):
        pd = {"pred_boxes": ref.make_lidar_boxes(seed, 40), "pred_scores": np.ones(40, np.float32), "pred_labels": np.ones(40, np.int64)}
        an = k.prediction_anno(pd, ref.make_calib(seed), meta["builder/%d" % seed]["image_shape"], names)
        cam = np.concatenate([an["location"], an["dimensions"], an["rotation_y"][:, None]], 1)
        np.testing.assert_allclose(cam, z["builder/%d/camera" % seed], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(an["bbox"], z["builder/%d/image" % seed], rtol=1e-5, atol=1e-5)
