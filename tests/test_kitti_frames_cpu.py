"""btcdet_amd/kitti_frames.py on the host, against what the reference's own KittiDataset.__getitem__, Calibration, get_fov_flag and
boxes3d_kitti_camera_to_lidar recorded over the synthetic KITTI directory of tests/golden/kitti_frames.npz (generator:
tests/golden/gen_kitti_frames_golden.py), which every test rebuilds under tmp_path.

Exact: the parsed matrices, names, frame ids, image shapes, the presence of road_plane, the kept rows of the crop -- by the host statement
(bytes) and by the numpy restatement of include/btcdet_hip_frames.h (kitti_frames_ref.restate_keep), which the fixture's decision margin
entitles to the reference's decisions.  gt_boxes and road_plane come out of BLAS / LAPACK (np.dot, np.linalg.inv, norm), which another
CPU may round differently: they are held to 4 x the deviation from a wider evaluation that the generator measured and stored."""
import ctypes
import os
import re

import numpy as np
import pytest

import kitti_frames_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["Car", "Pedestrian", "Cyclist"]


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    from btcdet_amd.kitti_frames import KittiFrames
    return KittiFrames(kr.build_dir(kr.gold(), tmp_path_factory.mktemp("kitti")), "train")


def test_calibration_parses_to_the_recorded_matrices(frames):
    g = kr.gold()
    assert len(frames) == kr.N_FRAMES and frames.sample_id_list == kr.FRAME_IDS
    for k in range(kr.N_FRAMES):
        c = frames.calib(k)
        for name in ("P2", "R0", "V2C"):
            got = getattr(c, name)
            assert got.dtype == np.float32 and got.tobytes() == g["f%d_ref_%s" % (k, name)].tobytes(), (k, name)
    from btcdet_amd.kitti_frames import Calibration
    again = Calibration({"P2": c.P2, "R0": c.R0, "Tr_velo2cam": c.V2C})        # the dict form
    assert again.P2 is c.P2 and again.V2C is c.V2C and again.fu == c.P2[0, 0] and again.cv == c.P2[1, 2]


def test_scene_gives_the_recorded_host_keys(frames):
    g = kr.gold()
    tol_box, tol_plane = 4.0 * float(g["dev_gt_boxes"]), 4.0 * float(g["dev_road_plane"])
    assert 0 < tol_box < 1e-4 and 0 < tol_plane < 1e-14
    for k in range(kr.N_FRAMES):
        s = frames.scene(k)
        assert "points" not in s and s["frame_id"] == str(g["f%d_ref_frame_id" % k]) == kr.FRAME_IDS[k]
        assert np.array_equal(s["image_shape"], g["f%d_ref_image_shape" % k]) and s["image_shape"].dtype == np.int32
        assert s["calib"] is frames.calib(k)
        want_names = g["f%d_ref_gt_names" % k]
        assert s["gt_names"].shape == want_names.shape and list(s["gt_names"]) == list(want_names), k
        want = g["f%d_ref_gt_boxes" % k]
        assert s["gt_boxes"].dtype == np.float32 and s["gt_boxes"].shape == want.shape
        err = float(np.abs(s["gt_boxes"].astype(np.float64) - want.astype(np.float64)).max())
        print("frame", k, "gt_boxes", want.shape, "worst difference %.3g (allowed %.3g)" % (err, tol_box))
        assert err <= tol_box
        assert ("road_plane" in s) == (("f%d_ref_road_plane" % k) in g), k
        if "road_plane" in s:
            want = g["f%d_ref_road_plane" % k]
            err = float(np.abs(s["road_plane"] - want).max())
            print("frame", k, "road_plane worst difference %.3g (allowed %.3g)" % (err, tol_plane))
            assert s["road_plane"].dtype == np.float64 and err <= tol_plane and s["road_plane"][1] < 0
            assert abs(np.linalg.norm(s["road_plane"][:3]) - 1.0) < 1e-15
    assert "DontCare" in list(kr.gold()["f0_anno_name"]) and "DontCare" not in list(frames.scene(0)["gt_names"])
    assert "road_plane" in frames.scene(0) and "road_plane" in frames.scene(1) and "road_plane" not in frames.scene(3)


def test_a_frame_without_annos_gets_the_placeholders(frames):
    k = kr.HAS_ANNOS.index(False)
    assert "annos" not in frames.infos[k]
    s = frames.scene(k)
    assert s["gt_names"].dtype == np.int32 and s["gt_names"].tolist() == [1]
    assert s["gt_boxes"].dtype == np.float32 and s["gt_boxes"].shape == (1, 7) and not s["gt_boxes"].any()
    assert "road_plane" not in s and kr.HAS_PLANE[k]          # its plane file exists and is not read, as in the reference


def test_fov_crop_host_equals_the_recorded_points(frames):
    g = kr.gold()
    for k in range(kr.N_FRAMES):
        got = frames.fov_crop_host(k)
        want = g["f%d_ref_points" % k]
        assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes(), k
        assert 0 <= want.shape[0] < 0.5 * max(g["f%d_points" % k].shape[0], 2)          # most rows lie outside the view
    from btcdet_amd.kitti_frames import KittiFrames
    raw = KittiFrames(frames.root, "train", fov_points_only=False).fov_crop_host(0)
    assert raw.tobytes() == g["f0_points"].tobytes()


def _blocks(frames, ks):
    from btcdet_amd.kitti_frames import calib_block
    return [calib_block(frames.calib(k), frames.image_shape(k)) for k in ks]


def test_restatement_of_the_header_keeps_the_recorded_rows(frames):
    g = kr.gold()
    assert 10.0 * max(g["dev_ref"][:2].max(), g["dev_restate"][:2].max()) < kr.PX_MARGIN
    assert 10.0 * max(g["dev_ref"][2], g["dev_restate"][2]) < kr.DEPTH_MARGIN
    pts = [g["f%d_points" % k] for k in range(kr.N_FRAMES)]
    offsets = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])])
    blocks = _blocks(frames, range(kr.N_FRAMES))
    for k in range(kr.N_FRAMES):
        assert blocks[k].dtype == np.float32 and blocks[k].shape == (32,) and not blocks[k][26:].any()
        assert blocks[k][24] == kr.IMAGE_SHAPES[k][1] and blocks[k][25] == kr.IMAGE_SHAPES[k][0]
        c = frames.calib(k)
        assert blocks[k][:12].tobytes() == np.dot(c.V2C.T, c.R0.T).tobytes() and blocks[k][12:24].tobytes() == c.P2.tobytes()
        assert pts[k][kr.restate_keep(pts[k], blocks[k])].tobytes() == g["f%d_ref_points" % k].tobytes(), k
    out, out_offsets, idx = kr.restate_crop(np.concatenate(pts), offsets, blocks)
    assert out.tobytes() == np.concatenate([g["f%d_ref_points" % k] for k in range(kr.N_FRAMES)]).tobytes()
    assert out_offsets.tolist() == np.concatenate([[0], np.cumsum([g["f%d_ref_points" % k].shape[0] for k in range(kr.N_FRAMES)])]).tolist()
    assert np.array_equal(np.concatenate(pts)[idx], out)


def test_exact_case_on_the_edges():
    from btcdet_amd.kitti_frames import Calibration, calib_block, get_fov_flag
    cal, shape, pts, expect = kr.exact_case()
    assert np.array_equal(kr.gold()["exact_keep"], expect)                    # what the reference's own lines decided
    c = Calibration(cal)
    with np.errstate(all="ignore"):
        assert np.array_equal(get_fov_flag(c.lidar_to_rect(pts[:, 0:3]), shape, c), expect)
    block = calib_block(c, shape)
    assert np.array_equal(kr.restate_keep(pts, block), expect)
    u, v, depth, r2 = kr.restate_project(pts, block)
    assert u[0] == 0 and u[1] == shape[1] and v[2] == shape[0] - 1 and depth[3] == 0 and r2[4] == 0 and np.isneginf(u[4]) and np.isnan(u[5])
    assert 0 <= u[6] < shape[1] and 0 <= v[6] < shape[0] and depth[6] < 0 and np.isnan(u[7])


def test_calib_block_refuses_what_float32_cannot_hold(frames):
    from btcdet_amd.kitti_frames import Calibration, calib_block
    c = frames.calib(0)
    calib_block(c, (2 ** 24 - 1, 2 ** 24 - 1))
    for shape in ((2 ** 24, 10), (10, 2 ** 24), (-1, 10)):
        with pytest.raises(ValueError):
            calib_block(c, shape)
    with pytest.raises(ValueError):
        calib_block(Calibration({"P2": c.P2.astype(np.float64), "R0": c.R0, "Tr_velo2cam": c.V2C}), (375, 1242))


def test_calibration_frame_changes(frames):
    """the remaining surface: a round trip, the image projection against float64, the corner boxes"""
    c = frames.calib(1)
    rng = np.random.default_rng(5)
    p = rng.uniform(-20, 20, (64, 3)).astype(np.float32)
    p[:, 0] = rng.uniform(5, 40, 64)
    rect = c.lidar_to_rect(p)
    assert rect.dtype == np.float32 and np.abs(c.rect_to_lidar(rect) - p).max() < 1e-4
    img, depth = c.lidar_to_img(p)
    u64, v64, d64 = kr.project64(p, c.lidar_to_rect_matrix(), c.P2)
    assert np.abs(img[:, 0] - u64).max() < 1e-2 and np.abs(img[:, 1] - v64).max() < 1e-2 and np.abs(depth - d64).max() < 1e-4
    back = c.img_to_rect(img[:, 0], img[:, 1], rect[:, 2])
    assert np.abs(back - rect).max() < 1e-2
    corners = rect[:8].reshape(1, 8, 3).astype(np.float64)
    boxes, pts2d = c.corners3d_to_img_boxes(corners)
    assert boxes.shape == (1, 4) and pts2d.shape == (1, 8, 2)
    h = np.hstack([corners[0], np.ones((8, 1))]) @ c.P2.astype(np.float64).T          # this one divides by the homogeneous coordinate
    x, y = h[:, 0] / h[:, 2], h[:, 1] / h[:, 2]
    assert np.allclose(boxes[0], [x.min(), y.min(), x.max(), y.max()], rtol=0, atol=1e-9) and np.allclose(pts2d[0], np.stack([x, y], 1), rtol=0, atol=1e-9)
    assert c.cart_to_hom(p).dtype == np.float32 and c.cart_to_hom(p).shape == (64, 4)


def test_evaluator_and_sampler_accept_a_calibration(frames):
    from btcdet_amd.database_sampler import DataBaseSampler
    from btcdet_amd.kitti_eval import KittiEvaluator, prediction_anno
    with_annos = [k for k in range(kr.N_FRAMES) if kr.HAS_ANNOS[k]]
    gts = frames.gt_annos(with_annos)
    assert [list(a["name"]) for a in gts] == [kr.NAMES[k] for k in with_annos]
    gts[0]["name"][0] = "changed"                                                   # a copy: the infos keep theirs
    assert frames.infos[with_annos[0]]["annos"]["name"][0] == kr.NAMES[with_annos[0]][0]
    ev = KittiEvaluator(frames.gt_annos(with_annos), CLASSES)
    preds = []
    for k in with_annos:
        s = frames.scene(k)
        n = s["gt_boxes"].shape[0]
        preds.append({"pred_boxes": s["gt_boxes"].copy(), "pred_scores": np.linspace(0.9, 0.5, n).astype(np.float32),
                      "pred_labels": np.array([CLASSES.index(x) + 1 if x in CLASSES else 1 for x in s["gt_names"]])})
    ev.add(frames.frame_ids(with_annos), preds, frames.calibs(with_annos), frames.image_shapes(with_annos))
    assert len(ev.dt_annos) == len(ev.gt_annos) == len(with_annos)
    for k, anno in zip(with_annos, ev.dt_annos):
        # a ground-truth box sent back through the detection route lands on its label: location, (l, h, w), rotation_y
        real = frames.infos[k]["annos"]["name"] != "DontCare"
        for key in ("location", "dimensions", "rotation_y"):
            assert np.abs(anno[key] - frames.infos[k]["annos"][key][real]).max() < 1e-4, (k, key)
        assert anno["frame_id"] == kr.FRAME_IDS[k]
    one = prediction_anno(preds[0], frames.calib(with_annos[0]), frames.image_shape(with_annos[0]), CLASSES)      # the object itself
    assert one["bbox"].shape == (preds[0]["pred_boxes"].shape[0], 4) and np.array_equal(one["bbox"], ev.dt_annos[0]["bbox"])
    # the sampler's road-plane step: the boxes land on the plane
    s = frames.scene(0)
    boxes = s["gt_boxes"].copy()
    moved, lift = DataBaseSampler.put_boxes_on_road_planes(boxes.copy(), s["road_plane"], s["calib"])
    a, b, c_, d = s["road_plane"]
    floor = moved[:, :3].copy()
    floor[:, 2] -= moved[:, 5] / 2
    cam = s["calib"].lidar_to_rect(floor)
    assert np.abs(a * cam[:, 0] + b * cam[:, 1] + c_ * cam[:, 2] + d).max() < 1e-4
    assert np.allclose(boxes[:, 2] - lift, moved[:, 2], atol=1e-6) and np.array_equal(moved[:, [0, 1, 3, 4, 5, 6]], boxes[:, [0, 1, 3, 4, 5, 6]])


# ------------------------------------------------------------------------------------------------------------------------- C ABI
def test_ctypes_table_matches_the_header():
    from btcdet_amd import _lib
    src = open(os.path.join(ROOT, "include", "btcdet_hip_frames.h")).read()
    for line in ("r_j   = ((x*M[0][j] + y*M[1][j]) + z*M[2][j]) + M[3][j]", "h_i   = ((r_0*P2[i][0] + r_1*P2[i][1]) + r_2*P2[i][2]) + P2[i][3]",
                 "u     = h_0 / r_2,  v = h_1 / r_2,  depth = h_2 - P2[2][3]", "keep  = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (depth >= 0)"):
        assert line in src, "the header states its formulas: " + line
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.FRAMES_EXPORTED_SYMBOLS) == ["btc_fov_crop", "btc_fov_crop_ws_bytes"]
    L = _lib.lib()
    kinds = {"int": _lib.ci, "size_t": _lib.sz}
    for n, count in (("btc_fov_crop", 13), ("btc_fov_crop_ws_bytes", 2)):
        assert hasattr(L, n)
        res, args = _lib._FRAMES_SIGS[n]
        m = re.search(r"(size_t|int)\s+%s\s*\(([^)]*)\)" % n, src)
        assert kinds[m.group(1)] is res, n
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args) == count, n
        for p, a in zip(params, args):
            want = _lib.vp if "*" in p else kinds[re.sub(r"\s+\w+$", "", p).replace("const ", "").strip()]
            assert a is want, (n, p)
    for other in ("btcdet_hip.h", "btcdet_hip_infer.h", "btcdet_hip_augment.h", "btcdet_hip_bestmatch.h"):
        assert "btc_fov_crop" not in open(os.path.join(ROOT, "include", other)).read()
    from btcdet_amd import kitti_frames
    assert kitti_frames.CALIB_FLOATS == int(re.search(r"#define BTC_FOV_CALIB_FLOATS (\d+)", src).group(1)) == 32


P = 0x1000      # a non-null address nobody reads: every call below returns from its argument checks


def test_argument_checks_return_before_any_launch():
    from btcdet_amd import _lib
    L = _lib.lib()
    assert L.btc_fov_crop_ws_bytes(-1, 1) == 0 and L.btc_fov_crop_ws_bytes(5, 0) == 0
    small, big = L.btc_fov_crop_ws_bytes(0, 1), L.btc_fov_crop_ws_bytes(120000, 2)
    assert 0 < small < big and L.btc_fov_crop_ws_bytes(120000, 200) == big and big >= 120000

    def call(pts=P, n=300, ld=4, offs=P, batch=2, calib=P, cap=300, out=P, out_offs=P, keep_idx=None, ws=P, ws_bytes=1 << 20):
        return L.btc_fov_crop(pts, n, ld, offs, batch, calib, cap, out, out_offs, keep_idx, ws, ws_bytes, None)
    for ld in (2, 0, -3):
        assert call(ld=ld) == -1 and b"ld >= 3" in L.btc_last_error(), ld
    for batch in (0, -1):
        assert call(batch=batch) == -1 and b"batch >= 1" in L.btc_last_error()
    assert call(n=-1, cap=0) == -1 and b"negative count" in L.btc_last_error()
    assert call(cap=299) == -1 and b"out_capacity 299 below n = 300" in L.btc_last_error()
    for kw in ("offs", "calib", "out_offs", "ws"):
        assert call(**{kw: None}) == -1 and b"missing pointer (scene_offsets, calib, out_offsets or ws)" in L.btc_last_error(), kw
    for kw in ("pts", "out"):
        assert call(**{kw: None}) == -1 and b"missing pointer (points or out)" in L.btc_last_error(), kw
    need = L.btc_fov_crop_ws_bytes(300, 2)
    for ws_bytes in (0, 8, need - 1):
        assert call(ws_bytes=ws_bytes) == -1 and b"workspace too small" in L.btc_last_error(), ws_bytes
    assert ctypes.sizeof(ctypes.c_float) * 32 == 128          # one calibration block is one 128-byte line
