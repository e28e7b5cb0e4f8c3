"""The ground-truth database: what btcdet_amd/gt_database.py and csrc/gt_database.hip are held to.

  * box_rows / restate_mask / restate_cut: include/btcdet_hip_gtdb.h in numpy, ONE np.float32 operation per rounded step -- the CPU-side
    pin of the kernel.  The mask is database_sampler.points_in_boxes_mask bit for bit (tests/test_gt_database_cpu.py asserts it).
  * local64: lx, ly, z - cz in float64 from the float32 boxes, with the reference's reading of the thresholds (dx / 2.0 + MARGIN in
    double, roiaware_pool3d.cpp:121-140): the yardstick of the decision margin.
  * the decision margin: a seeded point is redrawn while any of |lx|, |ly|, |z - cz| lies within FACE_MARGIN of its threshold for any
    box of its frame.  tests/golden/gen_gt_database_golden.py measures the worst float32 deviation from float64 and asserts that ten
    times it is below the margin; given that, the reference's compiled op, its transcription and the kernel owe the same decisions.
  * the synthetic KITTI directory of the golden file (frames(), build_dir()) on kitti_frames_ref's calibrations, and the exact case.
Imports nothing that needs a GPU."""
import os
import pickle

import numpy as np

import kitti_frames_ref as kr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "gt_database.npz")
F32 = np.float32
FACE_MARGIN = 1e-3             # metres: no sampled point lies closer to a face of a box of its frame
FRAME_IDS = ["000003", "000007", "000010", "000042", "000043"]
N_FRAMES = len(FRAME_IDS)
HAS_ANNOS = [True, True, False, True, True]
# names as the infos hold them; the boxes are the first `N_BOXES[k]` entries.  Frames 0, 1, 4: DontCare last, as real infos have.
# Frame 3: a DontCare BETWEEN real objects, so object 1 takes the name "DontCare" and object 2 "Pedestrian": the literal names[i].
NAMES = [["Car", "Pedestrian", "Car", "Car", "Cyclist", "DontCare", "DontCare"], ["Cyclist", "Van", "Car", "DontCare"], [],
         ["Car", "DontCare", "Pedestrian", "Car"], ["Car", "Car", "DontCare"]]
N_BOXES = [5, 3, 0, 3, 2]
BACKGROUND = [3001, 2300, 1700, 1100, 777]
CLUSTER = 70                   # rows drawn around each box, out to 1.2 x its extents


# ------------------------------------------------------------------------------------------------- include/btcdet_hip_gtdb.h in numpy
def box_rows(boxes):
    """(m, >= 7) boxes as given -> (m, 8) float32 rows: the float32 boxes (the reference passes boxes.float()), every value by the
    expression of database_sampler.points_in_boxes_mask"""
    b = np.asarray(boxes)[:, 0:7].astype(F32)
    half, margin = F32(2.0), F32(1e-2)
    hx = b[:, 3] / half
    hx = hx + margin
    hy = b[:, 4] / half
    hy = hy + margin
    hz = b[:, 5] / half
    neg = -b[:, 6]
    c, s = np.cos(neg).astype(F32), np.sin(neg).astype(F32)
    rows = np.stack([b[:, 0], b[:, 1], b[:, 2], hx, hy, hz, c, s], axis=1)
    assert rows.dtype == F32
    return rows


def restate_mask(points, row):
    """the header's test of every point against one (8) box row: one float32 operation per step"""
    p = np.asarray(points, F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore"):
        sx = x - row[0]
        sy = y - row[1]
        a = sx * row[6]
        b = sy * row[7]
        lx = a - b
        a = sx * row[7]
        b = sy * row[6]
        ly = a + b
        dz = z - row[2]
        assert lx.dtype == ly.dtype == dz.dtype == F32
        return (np.abs(dz) <= row[5]) & (np.abs(lx) < row[3]) & (np.abs(ly) < row[4])


def restate_cut(points, offsets, boxes_per_scene, centres=None):
    """btc_cut_objects: -> out (total, ld) f32 box-major, obj_offsets (m+1) i64, src_idx (total) i32"""
    points = np.asarray(points, F32)
    outs, idx, counts = [], [], []
    for s, boxes in enumerate(boxes_per_scene):
        boxes = np.asarray(boxes)
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        rows = box_rows(boxes) if boxes.shape[0] else np.zeros((0, 8), F32)
        ctr = np.asarray(boxes[:, 0:3] if centres is None else centres[s], np.float64).reshape(-1, 3)
        for j in range(rows.shape[0]):
            keep = np.flatnonzero(restate_mask(points[lo:hi], rows[j]))
            cut = points[lo:hi][keep].copy()
            cut[:, 0:3] = (cut[:, 0:3].astype(np.float64) - ctr[j]).astype(F32)
            outs.append(cut)
            idx.append(keep + lo)
            counts.append(keep.shape[0])
    out = np.concatenate(outs, axis=0) if outs else np.zeros((0, points.shape[1]), F32)
    src = np.concatenate(idx).astype(np.int32) if idx else np.zeros((0,), np.int32)
    return out, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), src


def local64(points, boxes):
    """-> (|lx|, |ly|, |z - cz|) (m, n) float64 and their thresholds (m, 1) as the reference's C++ reads them: the boxes rounded to
    float32 and widened, cos / sin in double, dx / 2.0 + MARGIN with MARGIN = (double)1e-2f"""
    p = np.asarray(points)[:, 0:3].astype(np.float64)
    b = np.asarray(boxes)[:, 0:7].astype(F32).astype(np.float64)
    sx, sy = p[None, :, 0] - b[:, None, 0], p[None, :, 1] - b[:, None, 1]
    c, s = np.cos(-b[:, 6])[:, None], np.sin(-b[:, 6])[:, None]
    margin = float(F32(1e-2))
    return (np.abs(sx * c - sy * s), np.abs(sx * s + sy * c), np.abs(p[None, :, 2] - b[:, None, 2])), \
           (b[:, 3:4] / 2.0 + margin, b[:, 4:5] / 2.0 + margin, b[:, 5:6] / 2.0)


def face_distance(points, boxes):
    """per point: the least distance (float64 metres) of |lx|, |ly|, |z - cz| from its threshold over all boxes; inf without boxes"""
    if np.asarray(boxes).shape[0] == 0:
        return np.full((np.asarray(points).shape[0],), np.inf)
    vals, thr = local64(points, boxes)
    return np.min([np.abs(v - t).min(axis=0) for v, t in zip(vals, thr)], axis=0)


def local32(points, boxes):
    """the float32 values the restatement compares (|lx|, |ly|, |z - cz|) and its thresholds, widened: for the measured deviation"""
    p = np.asarray(points, F32)
    vals, thr = ([], [], []), ([], [], [])
    for row in box_rows(boxes):
        sx, sy = p[:, 0] - row[0], p[:, 1] - row[1]
        for k, v in enumerate((np.abs(sx * row[6] - sy * row[7]), np.abs(sx * row[7] + sy * row[6]), np.abs(p[:, 2] - row[2]))):
            vals[k].append(v.astype(np.float64))
            thr[k].append([float(row[3 + k])])
    return tuple(np.stack(v) for v in vals), tuple(np.array(t) for t in thr)


# ------------------------------------------------------------------------------------------------------------ the synthetic directory
def boxes_of(k):
    """frame k's gt_boxes_lidar (N_BOXES[k], 7) float64.  Frame 0: box 1 overlaps box 0 (they share rows), box 3 floats above every
    row (an empty object), box 4 is a small box far from the scan that holds exactly one row."""
    rng = np.random.default_rng(6100 + k)
    n = N_BOXES[k]
    b = np.stack([rng.uniform(8, 50, n), rng.uniform(-20, 20, n), rng.uniform(-1.2, -0.4, n), rng.uniform(3.2, 4.6, n), rng.uniform(1.5, 1.9, n),
                  rng.uniform(1.4, 1.9, n), rng.uniform(-3.1, 3.1, n)], axis=1).reshape(n, 7)
    if k == 0:
        b[1, 0:3] = b[0, 0:3] + np.array([1.0, 0.3, 0.05])
        b[1, 6] = b[0, 6] + 0.2
        b[3, 2] = 9.0
        b[4] = [-20.0, 3.0, 0.5, 0.2, 0.2, 0.2, 0.7]
    return b


def _draw(rng, k, boxes, which):
    """which == -1: background rows over the scan's range; otherwise rows in box `which`'s frame out to 1.2 x its extents"""
    def draw(cnt):
        p = np.empty((cnt, 4), F32)
        if which < 0:
            p[:, 0], p[:, 1], p[:, 2] = rng.uniform(0, 60, cnt), rng.uniform(-30, 30, cnt), rng.uniform(-3.0, 1.5, cnt)
        else:
            b = boxes[which]
            loc = rng.uniform(-1.2, 1.2, (cnt, 3)) * (b[3:6] / 2)
            c, s = np.cos(b[6]), np.sin(b[6])
            p[:, 0], p[:, 1], p[:, 2] = b[0] + loc[:, 0] * c - loc[:, 1] * s, b[1] + loc[:, 0] * s + loc[:, 1] * c, b[2] + loc[:, 2]
        p[:, 3] = rng.uniform(0.0, 1.0, cnt)
        return p
    return draw


def sample_to_margin(draw, n, boxes):
    pts = draw(n)
    for _ in range(200):
        bad = np.flatnonzero(~(face_distance(pts, boxes) > FACE_MARGIN))
        if bad.size == 0:
            return pts
        pts[bad] = draw(bad.size)
    raise AssertionError("could not sample to the margin")


def points_of(k):
    rng = np.random.default_rng(6200 + k)
    boxes = boxes_of(k)
    parts = [sample_to_margin(_draw(rng, k, boxes, -1), BACKGROUND[k], boxes)]
    for j in range(boxes.shape[0]):
        if k == 0 and j == 3:
            continue                                            # the empty object
        if k == 0 and j == 4:
            one = np.array([[boxes[4, 0] + 0.03, boxes[4, 1] - 0.02, boxes[4, 2] + 0.04, 0.5]], F32)      # the object of one row
            assert face_distance(one, boxes).min() > FACE_MARGIN
            parts.append(one)
            continue
        parts.append(sample_to_margin(_draw(rng, k, boxes, j), CLUSTER, boxes))
    pts = np.concatenate(parts, axis=0)
    return pts[rng.permutation(pts.shape[0])]                   # objects' rows lie scattered through the scan, as in a real one


def annos_of(k):
    """the annos of an info as get_infos leaves them, with gt_boxes_lidar in float64"""
    rng = np.random.default_rng(6300 + k)
    names = NAMES[k]
    n = len(names)
    bbox = np.stack([rng.uniform(0, 500, n), rng.uniform(100, 200, n)], axis=1)
    bbox = np.concatenate([bbox, bbox + rng.uniform(30, 200, (n, 2))], axis=1).astype(np.float32)
    return {"name": np.array(names), "truncated": rng.choice([0.0, 0.1, 0.4], n), "occluded": rng.integers(0, 3, n).astype(np.float64),
            "alpha": rng.uniform(-3, 3, n), "bbox": bbox, "dimensions": rng.uniform(1.4, 4.6, (n, 3)), "location": rng.uniform(-10, 40, (n, 3)),
            "rotation_y": rng.uniform(-3.1, 3.1, n), "score": -np.ones(n, np.float64), "difficulty": rng.integers(-1, 3, n).astype(np.int32),
            "index": np.arange(n, dtype=np.int32), "num_points_in_gt": rng.integers(0, 300, N_BOXES[k]).astype(np.int32),
            "gt_boxes_lidar": boxes_of(k)}


ANNO_KEYS = ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score", "difficulty", "index",
             "num_points_in_gt", "gt_boxes_lidar")


def frames():
    """the synthetic directory as arrays: what the generator stores and build_dir() writes out"""
    g = {}
    for k in range(N_FRAMES):
        g["f%d_points" % k] = points_of(k)
        g["f%d_calib_txt" % k] = np.frombuffer(kr.calib_text(kr.calib_arrays(k)).encode(), np.uint8)
        if HAS_ANNOS[k]:
            for key, v in annos_of(k).items():
                g["f%d_anno_%s" % (k, key)] = v
    return g


def infos_of(g, annotated_only=False):
    infos = []
    for k in range(N_FRAMES):
        info = {"point_cloud": {"num_features": 4, "lidar_idx": FRAME_IDS[k]},
                "image": {"image_idx": FRAME_IDS[k], "image_shape": np.array(kr.IMAGE_SHAPES[k % len(kr.IMAGE_SHAPES)], np.int32)}}
        if ("f%d_anno_name" % k) in g:
            info["annos"] = {key: np.array(g["f%d_anno_%s" % (k, key)]) for key in ANNO_KEYS}
        if "annos" in info or not annotated_only:
            infos.append(info)
    return infos


def build_dir(g, root, split="train"):
    """write the directory the arrays `g` describe under `root`: training/{velodyne,calib}, ImageSets, kitti_infos_<split>.pkl (all
    frames) and kitti_infos_<split>_annotated.pkl (the reference raises on a frame without annos: it is given this one)"""
    root = str(root)
    for sub in ("training/velodyne", "training/calib", "ImageSets"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for k, fid in enumerate(FRAME_IDS):
        np.asarray(g["f%d_points" % k], F32).tofile(os.path.join(root, "training/velodyne/%s.bin" % fid))
        with open(os.path.join(root, "training/calib/%s.txt" % fid), "wb") as f:
            f.write(np.asarray(g["f%d_calib_txt" % k], np.uint8).tobytes())
    with open(os.path.join(root, "ImageSets/%s.txt" % split), "w") as f:
        f.write("".join(fid + "\n" for fid in FRAME_IDS))
    for name, only in (("kitti_infos_%s.pkl" % split, False), ("kitti_infos_%s_annotated.pkl" % split, True)):
        with open(os.path.join(root, name), "wb") as f:
            pickle.dump(infos_of(g, annotated_only=only), f)
    return root


_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(GOLD) as z:
            _gold = {k: z[k] for k in z.files}
    return _gold


DB_INFO_KEYS = ("name", "path", "image_idx", "gt_idx", "box3d_lidar", "num_points_in_gt", "difficulty", "bbox", "score")


def db_infos_as_arrays(db_infos, prefix):
    """a db_infos dict -> flat arrays (classes in order, then per class and key one stacked array) for the fixture"""
    out = {prefix + "classes": np.array(list(db_infos.keys()))}
    for name, entries in db_infos.items():
        for key in DB_INFO_KEYS:
            out["%s%s_%s" % (prefix, name, key)] = np.array([e[key] for e in entries])
    return out


def assert_db_infos_equal(db_infos, g, prefix):
    """db_infos against the arrays db_infos_as_arrays stored: classes in order, every entry, every key, value and dtype kind"""
    assert list(db_infos.keys()) == [str(c) for c in g[prefix + "classes"]], list(db_infos.keys())
    for name, entries in db_infos.items():
        for key in DB_INFO_KEYS:
            want = g["%s%s_%s" % (prefix, name, key)]
            got = np.array([e[key] for e in entries])
            assert got.shape == want.shape and got.dtype.kind == want.dtype.kind, (name, key, got.dtype, want.dtype)
            assert np.array_equal(got, want), (name, key)
        for e in entries:
            assert list(e.keys()) == list(DB_INFO_KEYS)


# --------------------------------------------------------------------------------------------------------------------- the exact case
def exact_case():
    """-> (boxes (1, 7) float32, points (n, 4) float32, expected inside (n) bool).  Heading 0 (c = 1, s = -0: lx = sx, ly = sy exactly),
    the centre on dyadic coordinates with cx = cy = 0, and dx, dy chosen (in the binade where 0.01f's low bits do so) so that fl32(d / 2 + 0.01f) rounds UP from the exact sum: a
    point AT that float32 value is outside and its lower neighbour inside under the float32 and under the double reading of the
    threshold alike.  Points exactly on a z face are inside (<=), and
    the rows just past one are chosen so that z - cz is exact in float32 (the C++ forms it in float as well).  Exempt from the margin -- its rows sit ON the faces."""
    def rounds_up(d):
        return float(F32(d) / F32(2.0) + F32(1e-2)) > float(F32(d)) / 2.0 + float(F32(1e-2))
    dx = next(d for d in (9.0, 10.0, 12.0) if rounds_up(d))
    dy = next(d for d in (8.5, 8.0, 11.0) if rounds_up(d))
    box = np.array([[0.0, 0.0, 0.5, dx, dy, 1.5, 0.0]], F32)
    hx, hy = F32(dx) / F32(2.0) + F32(1e-2), F32(dy) / F32(2.0) + F32(1e-2)
    lx, ly = np.nextafter(hx, F32(0)), np.nextafter(hy, F32(0))
    rows = [((hx, 0, 0.5), False), ((lx, 0, 0.5), True), ((-hx, 0, 0.5), False), ((-lx, 0, 0.5), True),
            ((0, hy, 0.5), False), ((0, ly, 0.5), True), ((0, -hy, 0.5), False), ((0, -ly, 0.5), True),
            ((0, 0, 1.25), True), ((0, 0, -0.25), True), ((0, 0, np.nextafter(F32(1.25), F32(2))), False),
            ((0, 0, F32(-0.25) - F32(2.0 ** -23)), False), ((lx, ly, 1.25), True), ((np.nan, 0, 0.5), False)]
    pts = np.array([list(p) + [0.125 * i] for i, (p, _) in enumerate(rows)], F32)
    return box, pts, np.array([k for _, k in rows])
