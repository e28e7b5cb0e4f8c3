"""The KITTI infos: what btcdet_amd/kitti_infos.py and csrc/kitti_infos.hip are held to.

  * hull_rows / restate_counts: btc_count_in_boxes of include/btcdet_hip_infos.h in numpy, ONE float32 operation per rounded step: the
    FOV decision is kitti_frames_ref.restate_keep, the in-box decision gt_database_ref.restate_mask over rows without the 0.01 margin.
  * restate_sphere / restate_cells: btc_coverage_cells in numpy, ONE float64 operation per rounded step, in the header's order.
  * the decision margins.  Counts: a scan row is redrawn while it lies within FACE_MARGIN of a bare face (dx / 2, no 0.01) of a box
    of its frame in float64, or within kitti_frames_ref's PX_MARGIN / DEPTH_MARGIN of the camera's view.  Cells: the generator
    measures the worst deviation of (s - mn) / res between the reference's numpy chain and the restatement and asserts that every
    value lies ten times that far from an integer.  tests/golden/gen_kitti_infos_golden.py measures and asserts both.
  * the synthetic KITTI directory of the golden file: label text, PNG bytes (zlib and struct, no image library), build_dir().
Imports nothing that needs a GPU."""
import os
import struct
import zlib

import numpy as np

import gt_database_ref as gr
import kitti_frames_ref as kr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "kitti_infos.npz")
F32 = np.float32
FACE_MARGIN = 1e-3             # metres: no sampled point lies closer to a bare face of a box of its frame
FRAME_IDS = ["000003", "000007", "000010", "000042", "000043"]
N_FRAMES = len(FRAME_IDS)
# DontCare rows last, as in real label files.  Frame 2: one object (coverage_rates of shape (1, 1)); frame 4: no object at all.
NAMES = [["Car", "Pedestrian", "Car", "Car", "Cyclist", "DontCare", "DontCare"], ["Cyclist", "Van", "Car", "DontCare"], ["Car"],
         ["Car", "Pedestrian", "Car", "DontCare"], ["DontCare"]]
BACKGROUND = [3001, 2300, 1700, 1100, 777]
CLUSTER = 70                   # rows drawn around each box, out to 1.2 x its extents
GREY = [False, False, True, False, False]      # frame 2's image is an 8-bit grey PNG, the others RGB
SPHERE_RES = np.array([0.32, 0.5184, 0.4203125])
COVERAGE_CLASSES = ("Car", "Pedestrian", "Cyclist")
INFO_ANNO_KEYS = ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score", "difficulty", "index",
                  "gt_boxes_lidar", "num_points_in_gt")
CALIB_KEYS = ("P2", "R0_rect", "Tr_velo_to_cam")


def image_hw(k):
    return kr.IMAGE_SHAPES[k % len(kr.IMAGE_SHAPES)]


# ----------------------------------------------------------------------------------------- btc_count_in_boxes in numpy (float32 steps)
def hull_rows(boxes):
    """(m, >= 7) boxes as given -> (m, 8) float32 rows: the float32 box, dx/2, dy/2, dz/2 (no margin), cos(-heading), sin(-heading)"""
    b = np.asarray(boxes)[:, 0:7].astype(F32)
    half = F32(2.0)
    hx = b[:, 3] / half
    hy = b[:, 4] / half
    hz = b[:, 5] / half
    neg = -b[:, 6]
    c, s = np.cos(neg).astype(F32), np.sin(neg).astype(F32)
    rows = np.stack([b[:, 0], b[:, 1], b[:, 2], hx, hy, hz, c, s], axis=1)
    assert rows.dtype == F32
    return rows


def restate_counts(points, offsets, blocks, boxes_per_scene):
    """-> counts (m) int32 box-major over the scenes, fov_rows (B) int32"""
    points = np.asarray(points, F32)
    counts, fov = [], []
    for s, boxes in enumerate(boxes_per_scene):
        p = points[int(offsets[s]):int(offsets[s + 1])]
        seen = kr.restate_keep(p, blocks[s]) if p.shape[0] else np.zeros((0,), bool)
        fov.append(int(seen.sum()))
        boxes = np.asarray(boxes)
        for row in (hull_rows(boxes) if boxes.shape[0] else ()):
            counts.append(int((seen & gr.restate_mask(p, row)).sum()) if p.shape[0] else 0)
    return np.array(counts, np.int32).reshape(-1), np.array(fov, np.int32)


def local64(points, boxes):
    """-> (|lx|, |ly|, |z - cz|) (m, n) float64 and the bare thresholds (m, 1), from the boxes AS GIVEN (float64: in_hull's corners come
    from them unrounded), cos / sin in double: the yardstick of the decision margin"""
    p = np.asarray(points)[:, 0:3].astype(np.float64)
    b = np.asarray(boxes)[:, 0:7].astype(np.float64)
    sx, sy = p[None, :, 0] - b[:, None, 0], p[None, :, 1] - b[:, None, 1]
    c, s = np.cos(-b[:, 6])[:, None], np.sin(-b[:, 6])[:, None]
    return (np.abs(sx * c - sy * s), np.abs(sx * s + sy * c), np.abs(p[None, :, 2] - b[:, None, 2])), (b[:, 3:4] / 2.0, b[:, 4:5] / 2.0, b[:, 5:6] / 2.0)


def local32(points, boxes):
    """the float32 values the restatement compares and its thresholds, widened"""
    p = np.asarray(points, F32)
    vals, thr = ([], [], []), ([], [], [])
    for row in hull_rows(boxes):
        sx, sy = p[:, 0] - row[0], p[:, 1] - row[1]
        for k, v in enumerate((np.abs(sx * row[6] - sy * row[7]), np.abs(sx * row[7] + sy * row[6]), np.abs(p[:, 2] - row[2]))):
            vals[k].append(v.astype(np.float64))
            thr[k].append([float(row[3 + k])])
    return tuple(np.stack(v) for v in vals), tuple(np.array(t) for t in thr)


def face_distance(points, boxes):
    """per point: the least float64 distance of |lx|, |ly|, |z - cz| from its bare threshold over all boxes; inf without boxes"""
    if np.asarray(boxes).shape[0] == 0:
        return np.full((np.asarray(points).shape[0],), np.inf)
    vals, thr = local64(points, boxes)
    return np.min([np.abs(v - t).min(axis=0) for v, t in zip(vals, thr)], axis=0)


def decide64(points, boxes):
    vals, thr = local64(points, boxes)
    return (vals[2] <= thr[2]) & (vals[0] < thr[0]) & (vals[1] < thr[1])


# ----------------------------------------------------------------------------------------- btc_coverage_cells in numpy (float64 steps)
def pose_of(box):
    """(7) float64 box -> [cx, cy, cz, cos(yaw), sin(yaw)] float64, as get_yaw_rotation takes them"""
    box = np.asarray(box, np.float64)
    return np.array([box[0], box[1], box[2], np.cos(box[6]), np.sin(box[6])], np.float64)


def restate_sphere(x, y, z):
    """-> (n, 3) float64: r, azimuth, elevation, one operation per step"""
    xx = x * x
    yy = y * y
    zz = z * z
    xy = xx + yy
    r = np.sqrt(xy + zz)
    az = np.arctan2(-y, x)
    az = az * 180.0
    az = az / np.pi
    el = np.arctan2(z, np.sqrt(xy))
    el = el * 180.0
    el = el / np.pi
    return np.stack([r, az, el], axis=-1)


def restate_template_sphere(tmpl, pose):
    t = np.asarray(tmpl, F32).reshape(-1, 3).astype(np.float64)
    a = t[:, 0] * pose[3]
    b = t[:, 1] * pose[4]
    d = t[:, 0] * pose[4]
    e = t[:, 1] * pose[3]
    return restate_sphere((a - b) + pose[0], (d + e) + pose[1], t[:, 2] + pose[2])


def restate_object_sphere(obj, pose):
    o = np.asarray(obj, F32)[:, 0:3].astype(np.float64)
    return restate_sphere(o[:, 0] + pose[0], o[:, 1] + pose[1], o[:, 2] + pose[2])


def restate_quotients(tmpl, obj, pose):
    """-> mn (3), template quotients (n, 3), object quotients (k, 3): (s - mn) / res before the floor"""
    st = restate_template_sphere(tmpl, pose)
    mn = np.minimum(st.min(axis=0), 0.0)
    qt = (st - mn) / SPHERE_RES
    so = restate_object_sphere(obj, pose) if np.asarray(obj).shape[0] else np.zeros((0, 3))
    return mn, qt, (so - mn) / SPHERE_RES


def restate_cells(tmpl, obj, pose, limit=1024.0):
    """-> (unique_obj, unique_bm, status): status 1 (and no counts) when some n_k > limit (None: the arithmetic alone, no key to fit)"""
    if np.asarray(tmpl).reshape(-1, 3).shape[0] == 0:
        return 0, 0, 0
    _, qt, qo = restate_quotients(tmpl, obj, pose)
    ct = np.floor(qt)
    n = ct.max(axis=0) + 11.0
    if limit is not None and not np.all(n <= limit):
        return None, None, 1
    unique_bm = len(np.unique(ct.astype(np.int64), axis=0))
    co = np.floor(qo)
    keep = np.all(co >= 0.0, axis=1) & np.all(co < n, axis=1)
    return len(np.unique(co[keep].astype(np.int64), axis=0)), unique_bm, 0


def restate_jobs(tmpl_rows, obj_rows, jobs, pose):
    """btc_coverage_cells over a job table -> cells (J, 2) int32 (flagged jobs left 0), status (J) int32"""
    jobs = np.asarray(jobs).reshape(-1, 4)
    cells, status = np.zeros((jobs.shape[0], 2), np.int32), np.zeros((jobs.shape[0],), np.int32)
    for j, (t0, tn, o0, on) in enumerate(jobs):
        uo, ub, st = restate_cells(tmpl_rows[t0:t0 + tn], obj_rows[o0:o0 + on], np.asarray(pose).reshape(-1, 5)[j])
        status[j] = st
        if st == 0:
            cells[j] = (uo, ub)
    return cells, status


# ------------------------------------------------------------------------------------------------------------ the synthetic directory
def png_bytes(h, w, grey=False):
    """a valid 8-bit PNG of h x w black pixels (RGB, or grey), written with zlib and struct"""
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    raw = (b"\x00" + b"\x00" * (w * (1 if grey else 3))) * h
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if grey else 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 9)) + \
        chunk(b"IEND", b"")


def want_boxes(k):
    """the lidar boxes frame k's labels are written from (gt_database_ref's, so frame 0 has two that overlap, one above every row and a
    small one behind the camera); get_infos recovers them from the label text to within its two decimals"""
    n = len([x for x in NAMES[k] if x != "DontCare"])
    return (gr.boxes_of(k) if k in (0, 1, 3) else gr.boxes_of(4))[:n]


# (bbox top, bbox bottom, truncation, occlusion): Easy, Moderate, Hard and the three ways to UnKnown
LEVELS = [(100.0, 150.0, 0.0, 0), (100.0, 130.0, 0.2, 1), (100.0, 126.0, 0.45, 2), (100.0, 120.0, 0.0, 0), (100.0, 160.0, 0.6, 0), (100.0, 160.0, 0.0, 3)]


def label_text(k):
    """frame k's label_2 text: the objects of want_boxes(k) in the camera frame, two decimals as KITTI prints them, every difficulty
    branch among them; frame 1's first line has a 16th field (a score); DontCare lines last"""
    c = kr.parse_calib(kr.calib_text(kr.calib_arrays(k)))
    M = kr.lidar_to_rect_matrix(c["R0"], c["Tr_velo2cam"]).astype(np.float64)
    rng = np.random.default_rng(6400 + k)
    lines = []
    boxes = want_boxes(k)
    for i, name in enumerate(NAMES[k]):
        left = rng.uniform(0, 900)
        if name == "DontCare":
            lines.append("DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10" % (left, 150.0, left + 60.0, 180.0))
            continue
        b = boxes[i]
        loc = np.array([b[0], b[1], b[2] - b[5] / 2, 1.0]) @ M
        top, bottom, trunc, occ = LEVELS[(i + k) % len(LEVELS)]
        line = "%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (
            name, trunc, occ, rng.uniform(-3, 3), left, top, left + rng.uniform(30, 200), bottom, b[5], b[4], b[3], loc[0], loc[1], loc[2],
            -b[6] - np.pi / 2)
        if k == 1 and i == 0:
            line += " 0.87"
        lines.append(line)
    return "\n".join(lines) + "\n"


def draw_scan(k, boxes):
    """frame k's scan around `boxes` (the gt_boxes_lidar get_infos derived): background rows all around the sensor and a cluster per box,
    every row redrawn to FACE_MARGIN of the bare faces and to kitti_frames_ref's margins of the camera's view, then shuffled"""
    c = kr.parse_calib(kr.calib_text(kr.calib_arrays(k)))
    M = kr.lidar_to_rect_matrix(c["R0"], c["Tr_velo2cam"])
    H, W = image_hw(k)
    rng = np.random.default_rng(6500 + k)

    def to_margin(draw, cnt):
        pts = draw(cnt)
        for _ in range(200):
            px, d = kr.edge_distance(pts, M, c["P2"], W, H)
            bad = np.flatnonzero(~((face_distance(pts, boxes) > FACE_MARGIN) & (px > kr.PX_MARGIN) & (d > kr.DEPTH_MARGIN)))
            if bad.size == 0:
                return pts
            pts[bad] = draw(bad.size)
        raise AssertionError("could not sample to the margins")

    def background(cnt):
        p = np.empty((cnt, 4), F32)
        p[:, 0], p[:, 1], p[:, 2], p[:, 3] = rng.uniform(-30, 60, cnt), rng.uniform(-30, 30, cnt), rng.uniform(-3.0, 1.5, cnt), rng.uniform(0, 1, cnt)
        return p

    def cluster(b):
        def draw(cnt):
            p = np.empty((cnt, 4), F32)
            loc = rng.uniform(-1.2, 1.2, (cnt, 3)) * (b[3:6] / 2)
            cs, sn = np.cos(b[6]), np.sin(b[6])
            p[:, 0], p[:, 1], p[:, 2] = b[0] + loc[:, 0] * cs - loc[:, 1] * sn, b[1] + loc[:, 0] * sn + loc[:, 1] * cs, b[2] + loc[:, 2]
            p[:, 3] = rng.uniform(0, 1, cnt)
            return p
        return draw

    parts = [to_margin(background, BACKGROUND[k])]
    for j in range(boxes.shape[0]):
        if k == 0 and j == 3:
            continue                                            # the box above every row
        parts.append(to_margin(cluster(boxes[j]), CLUSTER))
    pts = np.concatenate(parts, axis=0)
    return pts[rng.permutation(pts.shape[0])]


def draw_template(k, i, box):
    """a best-match template of object i of frame k: rows in the box's own frame, a little wider than the box (a completed shape
    reaches past the scan's rows); object 1 of frame 0 gets a template of ONE row, object 0 of frame 3 one of 30 equal rows"""
    rng = np.random.default_rng(6600 + 16 * k + i)
    n = 1 if (k, i) == (0, 1) else 30 if (k, i) == (3, 0) else int(rng.integers(60, 400))
    t = (rng.uniform(-0.55, 0.55, (n, 3)) * box[3:6]).astype(F32)
    if (k, i) == (3, 0):
        t[:] = t[0]
    return t


def dir_arrays(points):
    """the directory as arrays: what the generator stores and build_dir() writes out.  points: the scans, per frame"""
    g = {}
    for k in range(N_FRAMES):
        H, W = image_hw(k)
        g["f%d_points" % k] = np.asarray(points[k], F32)
        g["f%d_calib_txt" % k] = np.frombuffer(kr.calib_text(kr.calib_arrays(k)).encode(), np.uint8)
        g["f%d_label_txt" % k] = np.frombuffer(label_text(k).encode(), np.uint8)
        g["f%d_png" % k] = np.frombuffer(png_bytes(H, W, GREY[k]), np.uint8)
    return g


def build_dir(g, root, splits=None, test_frames=()):
    """write the raw directory the arrays `g` describe under `root`: training/{velodyne,calib,label_2,image_2} and ImageSets.
    splits: split name -> frame numbers (default: all five in `train`); test_frames: frame numbers copied to testing/ (no labels),
    listed in ImageSets/test.txt.  No pickle is written."""
    root = str(root)
    splits = {"train": list(range(N_FRAMES))} if splits is None else splits

    def put(sub, name, data):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
        with open(os.path.join(root, sub, name), "wb") as f:
            f.write(np.asarray(data, np.uint8).tobytes())

    for top, ks, labelled in (("training", sorted(set(sum((list(v) for v in splits.values()), []))), True), ("testing", list(test_frames), False)):
        for k in ks:
            fid = FRAME_IDS[k]
            os.makedirs(os.path.join(root, top, "velodyne"), exist_ok=True)
            np.asarray(g["f%d_points" % k], F32).tofile(os.path.join(root, top, "velodyne", "%s.bin" % fid))
            put(top + "/calib", "%s.txt" % fid, g["f%d_calib_txt" % k])
            put(top + "/image_2", "%s.png" % fid, g["f%d_png" % k])
            if labelled:
                put(top + "/label_2", "%s.txt" % fid, g["f%d_label_txt" % k])
    os.makedirs(os.path.join(root, "ImageSets"), exist_ok=True)
    for split, ks in list(splits.items()) + ([("test", list(test_frames))] if test_frames else []):
        with open(os.path.join(root, "ImageSets", "%s.txt" % split), "w") as f:
            f.write("".join(FRAME_IDS[k] + "\n" for k in ks))
    return root


# ---------------------------------------------------------------------------------------------------------------------- the fixture
def infos_as_arrays(infos, prefix):
    """a get_infos list -> flat arrays: per frame the key order of the info and of its annos, and every array"""
    out = {}
    for k, info in enumerate(infos):
        p = "%s%d_" % (prefix, k)
        out[p + "keys"] = np.array(list(info.keys()))
        out[p + "lidar_idx"] = np.array(info["point_cloud"]["lidar_idx"])
        out[p + "num_features"] = np.array(info["point_cloud"]["num_features"])
        out[p + "image_idx"] = np.array(info["image"]["image_idx"])
        out[p + "image_shape"] = info["image"]["image_shape"]
        for key in CALIB_KEYS:
            out[p + "calib_" + key] = info["calib"][key]
        if "annos" in info:
            out[p + "anno_keys"] = np.array(list(info["annos"].keys()))
            for key, v in info["annos"].items():
                out[p + "anno_" + key] = np.asarray(v)
    return out


def assert_infos_equal(infos, g, prefix, n_frames=None, frame_map=None):
    """infos against the arrays infos_as_arrays stored: key order, dtype, shape and value, exactly.  frame_map: info number -> stored
    frame number (default: the same)"""
    for k, info in enumerate(infos):
        p = "%s%d_" % (prefix, k if frame_map is None else frame_map[k])
        assert list(info.keys()) == [str(x) for x in g[p + "keys"]], (k, list(info.keys()))
        assert list(info["point_cloud"].keys()) == ["num_features", "lidar_idx"] and list(info["image"].keys()) == ["image_idx", "image_shape"]
        assert info["point_cloud"]["lidar_idx"] == str(g[p + "lidar_idx"]) and info["point_cloud"]["num_features"] == int(g[p + "num_features"])
        assert info["image"]["image_idx"] == str(g[p + "image_idx"])
        pairs = [("image_shape", info["image"]["image_shape"], g[p + "image_shape"])]
        assert list(info["calib"].keys()) == list(CALIB_KEYS)
        pairs += [("calib " + key, info["calib"][key], g[p + "calib_" + key]) for key in CALIB_KEYS]
        if "annos" in info:
            assert list(info["annos"].keys()) == [str(x) for x in g[p + "anno_keys"]], (k, list(info["annos"].keys()))
            pairs += [("annos " + key, info["annos"][key], g[p + "anno_" + key]) for key in info["annos"]]
        for what, got, want in pairs:
            assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (k, what, got.dtype, want.dtype, got.shape, want.shape)
            assert np.array_equal(got, want), (k, what)
    if n_frames is not None:
        assert len(infos) == n_frames


def template_arrays(g):
    """the stored templates as the dict TemplateBank.from_arrays takes: (class, image_idx, gt_idx) -> (n, 3) float32"""
    out = {}
    for key in g:
        if key.startswith("tmpl_"):
            _, k, i = key.split("_")
            k, i = int(k), int(i)
            out[(NAMES[k][i], int(FRAME_IDS[k]), i)] = np.asarray(g[key], F32)
    return out


_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(GOLD) as z:
            _gold = {k: z[k] for k in z.files}
    return _gold
