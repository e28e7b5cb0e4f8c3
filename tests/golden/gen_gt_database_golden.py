"""Golden vectors of the reference's ground-truth database (runs only where the reference is mounted): its OWN
KittiDataset.create_groundtruth_database (btcdet/datasets/kitti/kitti_dataset.py:267-317) over the synthetic KITTI directory of
tests/gt_database_ref.py, with the one compiled primitive it calls -- absent here -- served by the numpy transcription of
roiaware_pool3d.cpp:128-140 that gen_sampler_golden.py uses.

    python tests/golden/gen_gt_database_golden.py   ->  tests/golden/gt_database.npz

Stored: the directory's contents as arrays (tests rebuild it under tmp_path); every file the reference wrote (name and bytes, in
order) and every db_info field, in order, for used_classes=None ("all_") and used_classes=["Car"] ("car_"); the exact case's decisions.

The decision margin.  The reference's C++ compares in double against dx / 2.0 + MARGIN and takes cos / sin from libm; the project's
predicate forms everything in float32.  Per frame the generator measures the worst |float32 - float64| of |lx|, |ly|, |z - cz| and of
their thresholds (`dev`, stored), and ASSERTS that every point lies at least ten times that far from every face of every box of its
frame -- gt_database_ref.sample_to_margin draws to FACE_MARGIN, which must exceed it -- and that the float32 restatement, the
transcription and the double reading make the same decisions.  The exact case is exempt: its rows sit on the faces, and the
generator asserts its decisions under both readings."""
import os
import pickle
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
import torch  # noqa: E402
import gt_database_ref as gr  # noqa: E402


def points_in_boxes_cpu(boxes, pts, out):
    """the transcription of gen_sampler_golden.py"""
    b, p = boxes.numpy(), pts.numpy()
    sx, sy = p[None, :, 0] - b[:, None, 0], p[None, :, 1] - b[:, None, 1]
    c, s = np.cos(-b[:, 6]).astype(np.float32)[:, None], np.sin(-b[:, 6]).astype(np.float32)[:, None]
    lx, ly = sx * c - sy * s, sx * s + sy * c
    ok = (np.abs(p[None, :, 2] - b[:, None, 2]) <= b[:, None, 5] / np.float32(2.0)) & (np.abs(lx) < b[:, None, 3] / np.float32(2.0) + np.float32(1e-2)) & \
         (np.abs(ly) < b[:, None, 4] / np.float32(2.0) + np.float32(1e-2))
    out.copy_(torch.from_numpy(ok.astype(np.int32)))
    return 1


sys.modules["btcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda"].points_in_boxes_cpu = points_in_boxes_cpu
import btcdet.datasets.kitti.kitti_dataset as kitti_dataset  # noqa: E402
from btcdet.datasets.kitti.kitti_dataset import KittiDataset  # noqa: E402

if not hasattr(kitti_dataset, "Path"):      # the module imports Path only under __main__, where it calls this method
    kitti_dataset.Path = Path


def decide64(points, boxes):
    vals, thr = gr.local64(points, boxes)
    return (vals[2] <= thr[2]) & (vals[0] < thr[0]) & (vals[1] < thr[1])


def run_reference(d, used_classes):
    cfg = ref_env.EasyDict(DATA_SPLIT={"train": "train", "test": "val"}, INFO_PATH={"train": ["kitti_infos_train_annotated.pkl"], "test": []},
                           FOV_POINTS_ONLY=True)
    ds = KittiDataset(dataset_cfg=cfg, class_names=None, training=True, root_path=Path(d))
    before = set(os.listdir(d))
    ds.create_groundtruth_database(os.path.join(d, "kitti_infos_train_annotated.pkl"), used_classes=used_classes, split="train")
    assert set(os.listdir(d)) - before <= {"gt_database", "kitti_dbinfos_train.pkl"}
    with open(os.path.join(d, "kitti_dbinfos_train.pkl"), "rb") as f:
        return pickle.load(f)


def main():
    g = gr.frames()
    gold = dict(g)
    dev = np.zeros((gr.N_FRAMES,))
    nearest = np.inf
    for k in range(gr.N_FRAMES):
        if not gr.HAS_ANNOS[k]:
            continue
        pts, boxes = g["f%d_points" % k], g["f%d_anno_gt_boxes_lidar" % k]
        v64, t64 = gr.local64(pts, boxes)
        v32, t32 = gr.local32(pts, boxes)
        dev[k] = max(max(float(np.abs(a - b).max()) for a, b in zip(v32, v64)), max(float(np.abs(a - b).max()) for a, b in zip(t32, t64)))
        nearest = min(nearest, float(gr.face_distance(pts, boxes).min()))
        mask32 = np.stack([gr.restate_mask(pts, row) for row in gr.box_rows(boxes)])
        out = torch.zeros(mask32.shape, dtype=torch.int32)
        points_in_boxes_cpu(torch.from_numpy(boxes).float(), torch.from_numpy(pts[:, 0:3]).float(), out)
        assert np.array_equal(mask32, out.numpy() > 0), (k, "the restatement and the transcription disagree")
        assert np.array_equal(mask32, decide64(pts, boxes)), (k, "the float32 and the double reading disagree")
        print("frame %d: %d rows, %d boxes, rows per box %s, deviation %.3g m" % (k, pts.shape[0], boxes.shape[0], mask32.sum(axis=1).tolist(), dev[k]))
    need = 10.0 * dev.max()
    print("margin needed %.3g m; nearest point %.3g m; FACE_MARGIN %.3g m" % (need, nearest, gr.FACE_MARGIN))
    assert nearest > need and gr.FACE_MARGIN > need, "a point within the margin of a face"
    gold["dev"] = dev
    m0 = np.stack([gr.restate_mask(g["f0_points"], row) for row in gr.box_rows(g["f0_anno_gt_boxes_lidar"])])
    assert m0[3].sum() == 0 and m0[4].sum() == 1 and (m0[0] & m0[1]).sum() > 0, "frame 0: an empty object, one of one row, two that share rows"

    for prefix, used in (("all_", None), ("car_", ["Car"])):
        with tempfile.TemporaryDirectory() as d:
            gr.build_dir(g, d)
            infos = run_reference(d, used)
            names = []
            for info in gr.infos_of(g, annotated_only=True):      # the order the reference wrote them in
                for i in range(info["annos"]["gt_boxes_lidar"].shape[0]):
                    names.append("%s_%s_%d.bin" % (info["point_cloud"]["lidar_idx"], info["annos"]["name"][i], i))
            assert sorted(names) == sorted(os.listdir(os.path.join(d, "gt_database")))
            data = [np.fromfile(os.path.join(d, "gt_database", n), dtype=np.uint8) for n in names]
        if prefix == "all_":
            gold["file_names"] = np.array(names)
            gold["file_sizes"] = np.array([x.shape[0] for x in data], np.int64)
            gold["file_bytes"] = np.concatenate(data)
        else:       # the files do not depend on used_classes
            assert names == list(gold["file_names"]) and np.array_equal(np.concatenate(data), gold["file_bytes"])
        gold.update(gr.db_infos_as_arrays(infos, prefix))
        gr.assert_db_infos_equal(infos, gold, prefix)
        print(prefix, {k: len(v) for k, v in infos.items()}, "%d files, %d bytes" % (len(names), sum(x.shape[0] for x in data)))
    assert "DontCare" in list(gold["all_classes"]) and list(gold["car_classes"]) == ["Car"]

    # the exact case under both readings of the threshold
    box, pts, expect = gr.exact_case()
    out = torch.zeros((1, pts.shape[0]), dtype=torch.int32)
    points_in_boxes_cpu(torch.from_numpy(box), torch.from_numpy(pts[:, 0:3].copy()), out)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(out.numpy()[0] > 0, expect) and np.array_equal(decide64(pts, box)[0], expect)
        assert np.array_equal(gr.restate_mask(pts, gr.box_rows(box)[0]), expect)
    hx = float(gr.box_rows(box)[0, 3])
    assert hx > float(box[0, 3]) / 2.0 + float(np.float32(1e-2)), "fl32(dx / 2 + 0.01f) rounds up"
    gold["exact_inside"] = expect
    out_path = os.path.join(HERE, "gt_database.npz")
    np.savez_compressed(out_path, **gold)
    print("wrote gt_database.npz %.0f KB" % (os.path.getsize(out_path) / 1024))


if __name__ == "__main__":
    main()
