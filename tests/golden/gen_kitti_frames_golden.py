"""Golden vectors of the reference's KITTI frame path (runs only where the reference is mounted): its OWN KittiDataset.__getitem__
(btcdet/datasets/kitti/kitti_dataset.py:413-460) with prepare_data replaced by a capture, over the synthetic KITTI directory of
tests/kitti_frames_ref.py (seeded scans all around the sensor, a different calibration and image shape per frame, annos with DontCare,
planes for some frames, one frame without annos), and its own get_fov_flag / Calibration / boxes3d_kitti_camera_to_lidar.

    python tests/golden/gen_kitti_frames_golden.py   ->  tests/golden/kitti_frames.npz

Stored: the directory's contents as arrays (tests rebuild it under tmp_path) and, per frame, what the reference handed to prepare_data:
the cropped points, gt_boxes, gt_names, road_plane, frame_id, image_shape; the parsed calibration matrices; the exact case's kept rows.

The reference's np.dot goes through BLAS: the bits of its u, v, depth are not a contract, its DECISIONS are.  The generator measures
  dev_ref     the worst |float32 - float64| of the reference's u, v (pixels) and depth (metres) over all points of all frames,
  dev_restate the same for the one-operation-per-rounding restatement of include/btcdet_hip_frames.h (kitti_frames_ref.restate_project),
ASSERTS that every point lies farther than ten times the larger of the two from u = 0, u = W, v = 0, v = H (pixels) and depth = 0
(metres) -- kitti_frames_ref.sample_points draws to PX_MARGIN / DEPTH_MARGIN, which must exceed that -- and that the restatement keeps
exactly the reference's rows.  `bits_differ` counts the u / v / depth values whose bits differ between the two (information only).
The exact case (kitti_frames_ref.exact_case) is exempt from the margin: every intermediate of it is exact.
gt_boxes / road_plane: stored with the worst deviation of the reference's result from a wider evaluation (float64 for the float32
boxes, long double for the float64 plane, floored at half an ulp of the largest value); tests allow four times that."""
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_env  # noqa: E402
import oracle_spconv  # noqa: E402

ref_env.install(oracle_spconv)
import kitti_frames_ref as kr  # noqa: E402
from btcdet.datasets.kitti.kitti_dataset import KittiDataset  # noqa: E402
from btcdet.utils import box_utils, calibration_kitti  # noqa: E402


def boxes64(cam, calib):
    """boxes3d_kitti_camera_to_lidar in float64 from the same float32 inputs"""
    cam = cam.astype(np.float64)
    r0, v2c = np.eye(4), np.eye(4)
    r0[:3, :3], v2c[:3, :] = calib.R0.astype(np.float64), calib.V2C.astype(np.float64)
    hom = np.hstack([cam[:, :3], np.ones((cam.shape[0], 1))])
    xyz = (hom @ np.linalg.inv((r0 @ v2c).T))[:, :3]
    xyz[:, 2] += cam[:, 4] / 2
    return np.concatenate([xyz, cam[:, 3:4], cam[:, 5:6], cam[:, 4:5], -(cam[:, 6:7] + np.pi / 2)], axis=1)


def plane_wide(path):
    with open(path) as f:
        p = np.array([float(v) for v in f.readlines()[3].split()], np.longdouble)
    if p[1] > 0:
        p = -p
    return p / np.sqrt((p[:3] * p[:3]).sum())


def deviations(points, calib, shape):
    """-> (dev_ref [3], dev_restate [3], bits that differ, least pixel distance, least depth distance, kept by reference, by restatement)"""
    rect = calib.lidar_to_rect(points[:, 0:3])
    img, depth = calib.rect_to_img(rect)
    assert img.dtype == np.float32 and depth.dtype == np.float32
    M = np.dot(calib.V2C.T, calib.R0.T)
    block = kr.calib_block(M, calib.P2, shape[1], shape[0])
    u64, v64, d64 = kr.project64(points, M, calib.P2)
    u, v, d, _ = kr.restate_project(points, block)
    dev_ref = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in ((img[:, 0], u64), (img[:, 1], v64), (depth, d64))]
    dev_res = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in ((u, u64), (v, v64), (d, d64))]
    differ = sum(int((a.view(np.int32) != b.view(np.int32)).sum()) for a, b in ((img[:, 0].copy(), u), (img[:, 1].copy(), v), (depth, d)))
    px, dd = kr.edge_distance(points, M, calib.P2, shape[1], shape[0])
    return dev_ref, dev_res, differ, float(px.min()), float(dd.min()), KittiDataset.get_fov_flag(rect, shape, calib), kr.restate_keep(points, block)


def main():
    g = kr.frames()
    gold = dict(g)
    with tempfile.TemporaryDirectory() as d:
        kr.build_dir(g, d)
        cfg = ref_env.EasyDict(DATA_SPLIT={"train": "train", "test": "val"}, INFO_PATH={"train": ["kitti_infos_train.pkl"], "test": []},
                               FOV_POINTS_ONLY=True)
        ds = KittiDataset(dataset_cfg=cfg, class_names=None, training=True, root_path=Path(d))      # class_names None: no augmentor / processor
        ds._merge_all_iters_to_one_epoch = False
        ds.prepare_data = lambda data_dict: dict(data_dict)
        assert len(ds) == kr.N_FRAMES and ds.sample_id_list == kr.FRAME_IDS
        dev_ref, dev_res, differ, px_min, d_min = np.zeros(3), np.zeros(3), 0, np.inf, np.inf
        dev_box, dev_plane = 0.0, 0.0
        for k in range(kr.N_FRAMES):
            got = ds[k]
            calib, shape = got["calib"], got["image_shape"]
            assert type(calib) is calibration_kitti.Calibration
            pts = g["f%d_points" % k]
            a, b, n_diff, px, dd, keep_ref, keep_res = deviations(pts, calib, shape)
            dev_ref, dev_res, differ = np.maximum(dev_ref, a), np.maximum(dev_res, b), differ + n_diff
            px_min, d_min = min(px_min, px), min(d_min, dd)
            assert got["points"].tobytes() == pts[keep_ref].tobytes()
            assert np.array_equal(keep_ref, keep_res), (k, "the restatement and the reference disagree on a row")
            gold["f%d_ref_points" % k] = got["points"]
            gold["f%d_ref_frame_id" % k] = np.array(got["frame_id"])
            gold["f%d_ref_image_shape" % k] = np.asarray(shape)
            gold["f%d_ref_gt_names" % k] = np.asarray(got["gt_names"])
            gold["f%d_ref_gt_boxes" % k] = got["gt_boxes"]
            for name in ("P2", "R0", "V2C"):
                gold["f%d_ref_%s" % (k, name)] = getattr(calib, name)
            if kr.HAS_ANNOS[k]:
                assert got["gt_boxes"].dtype == np.float32 and "DontCare" not in list(got["gt_names"])
                an = {key: g["f%d_anno_%s" % (k, key)] for key in kr.ANNO_KEYS}
                real = an["name"] != "DontCare"
                cam = np.concatenate([an["location"][real], an["dimensions"][real], an["rotation_y"][real][:, None]], axis=1).astype(np.float32)
                assert np.array_equal(box_utils.boxes3d_kitti_camera_to_lidar(cam.copy(), calib), got["gt_boxes"])
                dev_box = max(dev_box, float(np.abs(got["gt_boxes"].astype(np.float64) - boxes64(cam, calib)).max()))
            assert ("road_plane" in got) == (kr.HAS_ANNOS[k] and kr.HAS_PLANE[k])
            if "road_plane" in got:
                gold["f%d_ref_road_plane" % k] = got["road_plane"]
                wide = plane_wide(os.path.join(d, "training/planes/%s.txt" % kr.FRAME_IDS[k]))
                dev_plane = max(dev_plane, float(np.abs(got["road_plane"].astype(np.longdouble) - wide).max()),
                                float(np.abs(got["road_plane"]).max()) * 2.0 ** -53)
            print("frame %d: %d of %d rows kept, gt_boxes %s, names %s, keys %s" % (k, got["points"].shape[0], pts.shape[0], got["gt_boxes"].shape,
                                                                                     list(got["gt_names"]), sorted(got)))
    # the decision margin
    need_px = 10.0 * max(dev_ref[0], dev_ref[1], dev_res[0], dev_res[1])
    need_d = 10.0 * max(dev_ref[2], dev_res[2])
    print("deviation reference u %.3g v %.3g px, depth %.3g m; restatement u %.3g v %.3g px, depth %.3g m" % (*dev_ref, *dev_res))
    print("margin needed %.3g px / %.3g m; nearest point %.3g px / %.3g m; %d u/v/depth values differ in bits" % (need_px, need_d, px_min, d_min, differ))
    assert px_min > need_px and d_min > need_d, "a point within the margin of an image edge or of the camera plane"
    assert kr.PX_MARGIN > need_px and kr.DEPTH_MARGIN > need_d
    gold.update(dev_ref=dev_ref, dev_restate=dev_res, bits_differ=np.array(differ), dev_gt_boxes=np.array(dev_box), dev_road_plane=np.array(dev_plane))
    print("gt_boxes deviation %.3g, road_plane deviation %.3g" % (dev_box, dev_plane))
    # the exact case, through the reference's own lines
    cal, shape, pts, expect = kr.exact_case()
    calib = calibration_kitti.Calibration(cal)
    keep = KittiDataset.get_fov_flag(calib.lidar_to_rect(pts[:, 0:3]), shape, calib)
    block = kr.calib_block(np.dot(calib.V2C.T, calib.R0.T), calib.P2, shape[1], shape[0])
    assert np.array_equal(keep, expect) and np.array_equal(kr.restate_keep(pts, block), expect), keep
    gold["exact_keep"] = keep
    out = os.path.join(HERE, "kitti_frames.npz")
    np.savez_compressed(out, **gold)
    print("wrote kitti_frames.npz %.0f KB" % (os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main()
