"""Golden vectors of the reference's KITTI infos (runs only where the reference is mounted): its OWN KittiDataset.get_infos
(btcdet/datasets/kitti/kitti_dataset.py:129-201, with the real scipy.spatial.Delaunay behind in_hull) and its OWN
create_info_file_with_coverage (204-264) over the synthetic KITTI directory of tests/kitti_infos_ref.py.

    python tests/golden/gen_kitti_infos_golden.py   ->  tests/golden/kitti_infos.npz

What stands in for absent pieces: skimage.io.imread is a PNG reader of this file (zlib and struct; the reference only takes .shape[:2]
of what it returns); the database the coverage step reads is written by the reference's create_groundtruth_database, whose one
compiled primitive is served by the numpy transcription gen_gt_database_golden.py uses.

Stored: the directory as arrays (tests rebuild it under tmp_path); every field of every info, in order ("info<k>_", and "test<k>_"
for has_label=False); the templates ("tmpl_<frame>_<object>"); coverage_rates per frame ("cov<k>"); the two cell counts per job
("cells", in job order); the measured deviations and distances ("count_dev", "count_nearest", "cell_dev", "cell_nearest").

The decision margins.  Counts: per frame the generator measures the worst |float32 - float64| of |lx|, |ly|, |z - cz| and of the bare
thresholds dx / 2 (`count_dev`) and ASSERTS that every row lies at least ten times that far from every face of every box of its
frame, that the float32 restatement and the double reading decide alike, and that the restatement's counts are the reference's.
The FOV-edge margin of gen_kitti_frames_golden.py applies unchanged (kitti_infos_ref.draw_scan draws to it).  Cells: the worst
deviation of (s - mn) / res between the reference's numpy chain and the restatement in the header's order (`cell_dev`), and the
ASSERTION that every such value of either side lies ten times that far from an integer; the rows that define mn are 0 on both sides
and excluded.  Given both, exact integers are owed by any route whose error is of that size -- the device's atan2 included."""
import copy
import os
import pickle
import struct
import sys
import tempfile
import zlib
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_env  # noqa: E402
import oracle_spconv  # noqa: E402

ref_env.install(oracle_spconv)
import torch  # noqa: E402
import kitti_frames_ref as kr  # noqa: E402
import kitti_infos_ref as ir  # noqa: E402
from gen_gt_database_golden import points_in_boxes_cpu  # noqa: E402  (installs the transcription and imports the reference's dataset)


def imread(path):
    """an 8-bit, non-interlaced PNG whose rows all have filter 0 -> (H, W) or (H, W, 3) uint8"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, head = 8, b"", None
    while at < len(data):
        n, tag = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", data[at + 8:at + 8 + n])
        if tag == b"IDAT":
            idat += data[at + 8:at + 8 + n]
        at += 12 + n
    w, h, depth, colour, _, _, interlace = head
    assert depth == 8 and colour in (0, 2) and interlace == 0
    c = 1 if colour == 0 else 3
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * c)
    assert not rows[:, 0].any()
    img = rows[:, 1:].reshape(h, w, c)
    return img[:, :, 0] if c == 1 else img


sys.modules["skimage.io"].imread = imread
sys.modules["skimage"].io = sys.modules["skimage.io"]
import btcdet.datasets.kitti.kitti_dataset as kitti_dataset  # noqa: E402
from btcdet.datasets.kitti.kitti_dataset import KittiDataset  # noqa: E402
from btcdet.utils import coords_utils, point_box_utils  # noqa: E402

kitti_dataset.io.imread = imread
CELL_FLOOR = 1e-9


def dataset(d):
    cfg = ref_env.EasyDict(DATA_SPLIT={"train": "train", "test": "val"}, INFO_PATH={"train": [], "test": []}, FOV_POINTS_ONLY=True)
    return KittiDataset(dataset_cfg=cfg, class_names=None, training=True, root_path=Path(d))


def reference_quotients(tmpl, obj, box):
    """(s - mn) / res of the reference's chain (kitti_dataset.py:246-251, 211-214) for the template and the object rows"""
    res = np.asarray([[0.32, 0.5184, 0.4203125]])
    bm = np.einsum("nj,ij->ni", tmpl.reshape([-1, 3])[:, :3].astype(np.float32), point_box_utils.get_yaw_rotation(box[6])) + box[:3].reshape(-1, 3)
    pts = obj[:, :3] + box[:3].reshape(-1, 3)
    st = coords_utils.absxyz_2_spherexyz_np(bm[..., :3])
    mn = np.minimum(np.min(st, axis=0, keepdims=False), np.array([0.0, 0.0, 0.0])).reshape(1, 3)
    so = coords_utils.absxyz_2_spherexyz_np(pts[..., :3]) if len(pts) else np.zeros((0, 3))
    return (st - mn) / res, (so - mn) / res


def main():
    gold = {}
    with tempfile.TemporaryDirectory() as d:
        # the lidar boxes as the reference derives them from the label text, before any scan exists
        empty = [np.zeros((0, 4), np.float32)] * ir.N_FRAMES
        ir.build_dir(ir.dir_arrays(empty), d)
        ds = dataset(d)
        first = ds.get_infos(num_workers=1, has_label=True, count_inside_pts=False)
        boxes = [info["annos"]["gt_boxes_lidar"] for info in first]
        for k in (0, 1, 2, 3):
            assert np.abs(boxes[k] - ir.want_boxes(k)).max() < 0.02, "the labels give the boxes they were written from, to two decimals"
        g = ir.dir_arrays([ir.draw_scan(k, boxes[k]) for k in range(ir.N_FRAMES)])
        gold.update(g)
        ir.build_dir(g, d)
        infos = ds.get_infos(num_workers=1, has_label=True, count_inside_pts=True)
        test_infos = ds.get_infos(num_workers=1, has_label=False, count_inside_pts=False)
        plain = ds.get_infos(num_workers=1, has_label=True, count_inside_pts=False)
        assert all("num_points_in_gt" not in x["annos"] for x in plain) and all("annos" not in x for x in test_infos)

        # ---- counts: deviation, margin, decisions
        dev, nearest = np.zeros((ir.N_FRAMES,)), np.inf
        for k, info in enumerate(infos):
            pts, b = g["f%d_points" % k], boxes[k]
            assert np.array_equal(info["annos"]["gt_boxes_lidar"], b) and b.dtype == np.float64
            H, W = info["image"]["image_shape"]
            assert (H, W) == ir.image_hw(k)
            c = kr.parse_calib(kr.calib_text(kr.calib_arrays(k)))
            M = kr.lidar_to_rect_matrix(c["R0"], c["Tr_velo2cam"])
            block = kr.calib_block(M, c["P2"], W, H)
            seen = kr.restate_keep(pts, block)
            px, depth = kr.edge_distance(pts, M, c["P2"], W, H)
            assert px.min() > kr.PX_MARGIN and depth.min() > kr.DEPTH_MARGIN
            if b.shape[0]:
                v64, t64 = ir.local64(pts, b)
                v32, t32 = ir.local32(pts, b)
                dev[k] = max(max(float(np.abs(a - bb).max()) for a, bb in zip(v32, v64)), max(float(np.abs(a - bb).max()) for a, bb in zip(t32, t64)))
                nearest = min(nearest, float(ir.face_distance(pts, b).min()))
                mask32 = np.stack([ir.gr.restate_mask(pts, row) for row in ir.hull_rows(b)])
                assert np.array_equal(mask32, ir.decide64(pts, b)), (k, "the float32 and the double reading disagree")
            counts, fov = ir.restate_counts(pts, [0, pts.shape[0]], [block], [b])
            want = info["annos"]["num_points_in_gt"]
            assert want.dtype == np.int32 and np.array_equal(want[:b.shape[0]], counts) and np.all(want[b.shape[0]:] == -1), (k, want, counts)
            assert fov[0] == int(seen.sum())
            print("frame %d: %d rows, %d in view, points in gt %s, deviation %.3g m" % (k, pts.shape[0], fov[0], want.tolist(), dev[k]))
        need = 10.0 * dev.max()
        print("counts: margin needed %.3g m; nearest row %.3g m; FACE_MARGIN %.3g m" % (need, nearest, ir.FACE_MARGIN))
        assert nearest > need and ir.FACE_MARGIN > need, "a row within the margin of a bare face"
        n0 = infos[0]["annos"]["num_points_in_gt"]
        assert n0[3] == 0 and n0[4] == 0 and n0[0] > 0 and n0[1] > 0, "frame 0: a box above every row, a box behind the camera"
        gold.update(count_dev=dev, count_nearest=np.array(nearest))
        gold.update(ir.infos_as_arrays(infos, "info"))
        gold.update(ir.infos_as_arrays(test_infos, "test"))
        ir.assert_infos_equal(infos, gold, "info", n_frames=ir.N_FRAMES)
        levels = np.concatenate([x["annos"]["difficulty"] for x in infos])
        assert set(levels.tolist()) == {-1, 0, 1, 2} and infos[1]["annos"]["score"][0] == 0.87 and infos[0]["annos"]["score"][0] == -1.0

        # ---- coverage: the reference's database, template pickles, create_info_file_with_coverage
        info_path = os.path.join(d, "kitti_infos_train.pkl")
        with open(info_path, "wb") as f:
            pickle.dump(infos, f)
        ds.create_groundtruth_database(info_path, used_classes=None, split="train")
        roots = {name: Path(d) / ("bm_" + name) for name in ir.COVERAGE_CLASSES}
        for r in roots.values():
            r.mkdir()
        jobs = []
        for k, info in enumerate(infos):
            for i, name in enumerate(info["annos"]["name"]):
                if name in ir.COVERAGE_CLASSES:
                    t = ir.draw_template(k, i, boxes[k][i])
                    gold["tmpl_%d_%d" % (k, i)] = t
                    with open(roots[name] / ("%d_%d.pkl" % (int(ir.FRAME_IDS[k]), i)), "wb") as f:
                        pickle.dump(t, f)
                    jobs.append((k, i, name))
        ds.kitti_infos = copy.deepcopy(infos)
        covered = ds.create_info_file_with_coverage(roots, Path(d) / "gt_database", num_workers=1)
        cells, cell_dev, cell_nearest = [], 0.0, np.inf
        for k, i, name in jobs:
            t, box = gold["tmpl_%d_%d" % (k, i)], boxes[k][i]
            obj = np.fromfile(os.path.join(d, "gt_database", "%s_%s_%d.bin" % (ir.FRAME_IDS[k], name, i)), dtype=np.float32).reshape(-1, 4)
            rt, ro = reference_quotients(t, obj, box)
            _, qt, qo = ir.restate_quotients(t, obj, ir.pose_of(box))
            for a, b in ((rt, qt), (ro, qo)):
                if a.size == 0:
                    continue
                cell_dev = max(cell_dev, float(np.abs(a - b).max()))
                for q in (a, b):
                    live = q[~((a == 0) & (b == 0))]          # the rows that define mn: exactly 0 on both sides
                    if live.size:
                        cell_nearest = min(cell_nearest, float(np.abs(live - np.round(live)).min()))
            uo, ub, st = ir.restate_cells(t, obj, ir.pose_of(box))
            rate = covered[k]["annos"]["coverage_rates"].reshape(-1)[i]
            assert st == 0 and rate == uo / max(1, ub), (k, i, rate, uo, ub)
            cells.append((uo, ub))
            print("frame %d object %d %s: %d template rows, %d object rows, cells %d / %d" % (k, i, name, t.shape[0], obj.shape[0], uo, ub))
        print("cells: deviation %.3g; nearest to an integer %.3g" % (cell_dev, cell_nearest))
        # where the two numpy chains agree to the bit (deviation 0) the measured margin says nothing about another libm: the floor
        # CELL_FLOOR = 1e-9 cells is ~2000 ulp of the largest quotient (705 cells), far above an atan2 or sqrt that errs by a few ulp
        assert cell_nearest > max(10.0 * cell_dev, CELL_FLOOR), "a quotient within the margin of an integer"
        gold.update(cells=np.array(cells, np.int32), cell_dev=np.array(cell_dev), cell_nearest=np.array(cell_nearest))
        for k, info in enumerate(covered):
            assert list(info["annos"].keys())[-1] == "coverage_rates"
            gold["cov%d" % k] = info["annos"]["coverage_rates"]
            print("frame %d coverage_rates %s %s" % (k, info["annos"]["coverage_rates"].shape, info["annos"]["coverage_rates"].dtype))
        shapes = [gold["cov%d" % k].shape for k in range(ir.N_FRAMES)]
        assert (1, 1) in shapes and any(len(s) == 1 for s in shapes)
    out_path = os.path.join(HERE, "kitti_infos.npz")
    np.savez_compressed(out_path, **gold)
    print("wrote kitti_infos.npz %.0f KB" % (os.path.getsize(out_path) / 1024))


if __name__ == "__main__":
    main()
