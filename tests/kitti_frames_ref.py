"""KITTI frames and the field-of-view crop: what btcdet_amd/kitti_frames.py and csrc/fov_crop.hip are held to.

  * restate_keep / restate_crop: include/btcdet_hip_frames.h in numpy, ONE np.float32 operation per rounded step -- the CPU-side pin of
    the kernel's formulas.  The reference's own np.dot goes through BLAS (summation order and FMA use undefined), so the kernel is held
    to these formulas bit for bit and, through the decision margin below, to the reference's kept rows.
  * project64: the same projection in float64, the yardstick of both deviations and of the margin.
  * the decision margin: a seeded point is redrawn while its float64 u or v lies within PX_MARGIN of an image edge or its depth within
    DEPTH_MARGIN of 0.  tests/golden/gen_kitti_frames_golden.py measures the worst float32 deviation of the reference and of the
    restatement from float64 and asserts that ten times the larger one is below these margins (the factor the occupancy fixture uses:
    two float32 routes err independently); given that, both owe the same decisions, and exact kept-row sets are a fair demand.
  * the synthetic KITTI directory of the golden file (frames(), build_dir()) and the hand-made exact case (exact_case()).
Imports nothing that needs a GPU."""
import os
import pickle

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "kitti_frames.npz")
F32 = np.float32
PX_MARGIN = 0.125            # pixels: no sampled point projects closer to an image edge ...
DEPTH_MARGIN = 1.0         # metres: ... or lies closer to the camera plane (which also bounds |u|, |v| and with them their float32 ulp)
N_FRAMES = 4
ANNO_KEYS = ("name", "truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score", "difficulty", "index")


# --------------------------------------------------------------------------------------------------- include/btcdet_hip_frames.h in numpy
def calib_block(M, P2, W, H):
    b = np.zeros((32,), F32)
    b[0:12], b[12:24], b[24], b[25] = np.asarray(M, F32).reshape(-1), np.asarray(P2, F32).reshape(-1), W, H
    return b


def restate_project(points, block):
    """-> u, v, depth, r_2 (float32 arrays): every product and every sum its own float32 operation, in the header's order"""
    p = np.asarray(points, F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    M, P2 = block[0:12].reshape(4, 3), block[12:24].reshape(3, 4)
    with np.errstate(all="ignore"):
        r = []
        for j in range(3):
            a = x * M[0, j]
            b = y * M[1, j]
            s = a + b
            c = z * M[2, j]
            s = s + c
            r.append(s + M[3, j])
        h = []
        for i in range(3):
            a = r[0] * P2[i, 0]
            b = r[1] * P2[i, 1]
            s = a + b
            c = r[2] * P2[i, 2]
            s = s + c
            h.append(s + P2[i, 3])
        u = h[0] / r[2]
        v = h[1] / r[2]
        depth = h[2] - P2[2, 3]
    assert all(q.dtype == F32 for q in (u, v, depth))
    return u, v, depth, r[2]


def restate_keep(points, block):
    u, v, depth, _ = restate_project(points, block)
    with np.errstate(invalid="ignore"):
        return (u >= 0) & (u < block[24]) & (v >= 0) & (v < block[25]) & (depth >= 0)


def restate_crop(points, offsets, blocks):
    """btc_fov_crop: -> out (n', ld), out_offsets (B+1) i32, keep_idx (n') i32"""
    points = np.asarray(points, F32)
    keep = np.zeros((points.shape[0],), bool)
    for b in range(len(offsets) - 1):
        keep[offsets[b]:offsets[b + 1]] = restate_keep(points[offsets[b]:offsets[b + 1]], blocks[b])
    idx = np.flatnonzero(keep).astype(np.int32)
    out_offsets = np.array([int(keep[:o].sum()) for o in offsets], np.int32)
    return points[idx], out_offsets, idx


def project64(points, M, P2):
    """-> u, v, depth in float64 from float32 inputs (the matrices as given, widened)"""
    p = np.asarray(points)[:, :3].astype(np.float64)
    M, P2 = np.asarray(M, np.float64), np.asarray(P2, np.float64)
    r = p @ M[:3] + M[3]
    h = r @ P2[:, :3].T + P2[:, 3]
    with np.errstate(all="ignore"):
        return h[:, 0] / r[:, 2], h[:, 1] / r[:, 2], h[:, 2] - P2[2, 3]


def edge_distance(points, M, P2, W, H):
    """per point: (pixels to the nearest image edge in u or v, metres to the camera plane), float64"""
    u, v, d = project64(points, M, P2)
    px = np.minimum(np.minimum(np.abs(u), np.abs(u - W)), np.minimum(np.abs(v), np.abs(v - H)))
    return px, np.abs(d)


def lidar_to_rect_matrix(R0, V2C):
    """np.dot(V2C.T, R0.T) in float32, as Calibration.lidar_to_rect forms it"""
    return np.dot(np.asarray(V2C, F32).T, np.asarray(R0, F32).T)


def sample_points(rng, n, M, P2, W, H, ld=4, spread=60.0):
    """n seeded rows all around the sensor (most of them outside the camera's view, half of them behind it), redrawn to the margin"""
    def draw(k):
        p = np.empty((k, ld), F32)
        p[:, 0] = rng.uniform(-spread, spread, k)
        p[:, 1] = rng.uniform(-spread, spread, k)
        p[:, 2] = rng.uniform(-3.0, 1.5, k)
        p[:, 3:] = rng.uniform(0.0, 1.0, (k, ld - 3))
        return p
    pts = draw(n)
    for _ in range(200):
        px, d = edge_distance(pts, M, P2, W, H)
        bad = np.flatnonzero(~((px > PX_MARGIN) & (d > DEPTH_MARGIN)))      # (a NaN distance is bad too)
        if bad.size == 0:
            return pts
        pts[bad] = draw(bad.size)
    raise AssertionError("could not sample to the margin")


# ------------------------------------------------------------------------------------------------------------ the synthetic directory
def calib_arrays(k):
    """KITTI-like calibration of frame k (different per frame), float64 before it is printed"""
    rng = np.random.default_rng(7000 + k)
    f = 707.0493 + 14.3 * k
    P2 = np.array([[f, 0.0, 604.0814 + 3.1 * k, 45.75831 - 0.9 * k], [0.0, f, 180.5066 - 2.2 * k, -0.3454157 + 0.05 * k],
                   [0.0, 0.0, 1.0, 0.004981016 - 0.0004 * k]])
    P3 = P2.copy()
    P3[0, 3] -= 380.0
    a = rng.uniform(-0.02, 0.02, 3)                                # small rotations about the nominal axes
    def rot(ax, t):
        c, s = np.cos(t), np.sin(t)
        m = np.eye(3)
        i, j = [(1, 2), (0, 2), (0, 1)][ax]
        m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
        return m
    R0 = rot(0, a[0] / 2) @ rot(1, a[1] / 2) @ rot(2, a[2] / 2)
    axes = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])        # camera x = -lidar y, y = -lidar z, z = lidar x
    V2C = np.hstack([rot(0, a[2]) @ rot(2, a[0]) @ axes, np.array([[-0.004069766 + 0.01 * k], [-0.07631618], [-0.2717806 - 0.01 * k]])])
    return {"P2": P2, "P3": P3, "R0": R0, "Tr_velo2cam": V2C}


def calib_text(c):
    """the six lines of a KITTI calib file"""
    def line(name, m):
        return name + ": " + " ".join("%.12e" % v for v in np.asarray(m).reshape(-1))
    P0 = c["P2"].copy()
    P0[:, 3] = 0
    return "\n".join([line("P0", P0), line("P1", P0), line("P2", c["P2"]), line("P3", c["P3"]), line("R0_rect", c["R0"]),
                      line("Tr_velo_to_cam", c["Tr_velo2cam"]), line("Tr_imu_to_velo", np.eye(3, 4))]) + "\n"


IMAGE_SHAPES = [(375, 1242), (370, 1224), (374, 1238), (376, 1241)]
FRAME_IDS = ["000003", "000007", "000010", "000042"]
N_POINTS = [4096, 2500, 769, 1]
HAS_PLANE = [True, True, True, False]        # frame 2 has no annos: its plane file is never read
HAS_ANNOS = [True, True, False, True]
NAMES = [["Car", "DontCare", "Pedestrian", "Car", "DontCare"], ["Cyclist", "Van"], [], ["DontCare", "Car", "DontCare"]]


def parse_calib(text):
    """float32 matrices of a calib text, by the rule of the calib files (lines 2..5, the name dropped)"""
    rows = [np.array(line.strip().split(" ")[1:], dtype=F32) for line in text.splitlines()[2:6]]
    return {"P2": rows[0].reshape(3, 4), "P3": rows[1].reshape(3, 4), "R0": rows[2].reshape(3, 3), "Tr_velo2cam": rows[3].reshape(3, 4)}


def annos(k):
    """the `annos` of an info as get_infos leaves them (the keys __getitem__ and the evaluator read), DontCare rows last-or-between"""
    rng = np.random.default_rng(8000 + k)
    names = NAMES[k]
    n = len(names)
    real = np.array([x != "DontCare" for x in names])
    loc = np.stack([rng.uniform(-10, 10, n), rng.uniform(1.2, 2.0, n), rng.uniform(6, 45, n)], axis=1)
    dims = np.stack([rng.uniform(3.2, 4.6, n), rng.uniform(1.4, 1.9, n), rng.uniform(1.5, 1.9, n)], axis=1)     # l, h, w
    loc[~real], dims[~real] = -1000.0, -1.0
    bbox = np.stack([rng.uniform(0, 500, n), rng.uniform(100, 200, n)], axis=1)
    bbox = np.concatenate([bbox, bbox + rng.uniform(30, 200, (n, 2))], axis=1)
    index, cnt = [], 0
    for r in real:
        index.append(cnt if r else -1)
        cnt += int(r)
    return {"name": np.array(names), "truncated": np.where(real, rng.choice([0.0, 0.1, 0.4], n), -1.0), "occluded": np.where(real, rng.integers(0, 3, n), -1).astype(np.float64),
            "alpha": np.where(real, rng.uniform(-3, 3, n), -10.0), "bbox": bbox, "dimensions": dims, "location": loc,
            "rotation_y": np.where(real, rng.uniform(-3.1, 3.1, n), -10.0), "score": np.full((n,), -1.0), "difficulty": np.where(real, rng.integers(0, 3, n), -1).astype(np.int32),
            "index": np.array(index, np.int32)}


def plane_text(k):
    """a planes/*.txt: three header lines, then a b c d; frame 1's normal points down (b > 0) and is not of unit length, so the sign flip
    and the normalisation both act"""
    p = [[-0.007051, -0.999750, -0.021223, 1.680367], [0.0141, 1.9995, 0.0424, -3.3607], [-0.01, -0.9998, 0.02, 1.7], None][k]
    return "# Plane\nWidth 4\nHeight 1\n" + " ".join("%.6e" % v for v in p) + "\n"


def frames():
    """the synthetic directory as arrays: what the generator stores and build_dir() writes out"""
    g = {}
    for k in range(N_FRAMES):
        text = calib_text(calib_arrays(k))
        c = parse_calib(text)
        H, W = IMAGE_SHAPES[k]
        pts = sample_points(np.random.default_rng(9000 + k), N_POINTS[k], lidar_to_rect_matrix(c["R0"], c["Tr_velo2cam"]), c["P2"], W, H)
        g["f%d_points" % k] = pts
        g["f%d_calib_txt" % k] = np.frombuffer(text.encode(), np.uint8)
        if HAS_PLANE[k]:
            g["f%d_plane_txt" % k] = np.frombuffer(plane_text(k).encode(), np.uint8)
        if HAS_ANNOS[k]:
            for key, v in annos(k).items():
                g["f%d_anno_%s" % (k, key)] = v
    return g


def infos_of(g):
    infos = []
    for k in range(N_FRAMES):
        info = {"point_cloud": {"num_features": 4, "lidar_idx": FRAME_IDS[k]},
                "image": {"image_idx": FRAME_IDS[k], "image_shape": np.array(IMAGE_SHAPES[k], np.int32)}}
        if ("f%d_anno_name" % k) in g:
            info["annos"] = {key: np.array(g["f%d_anno_%s" % (k, key)]) for key in ANNO_KEYS}
        infos.append(info)
    return infos


def build_dir(g, root, split="train"):
    """write the directory the arrays `g` describe under `root`: training/{velodyne,calib,planes}, ImageSets, kitti_infos_<split>.pkl"""
    root = str(root)
    for sub in ("training/velodyne", "training/calib", "training/planes", "ImageSets"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for k, fid in enumerate(FRAME_IDS):
        np.asarray(g["f%d_points" % k], F32).tofile(os.path.join(root, "training/velodyne/%s.bin" % fid))
        with open(os.path.join(root, "training/calib/%s.txt" % fid), "wb") as f:
            f.write(np.asarray(g["f%d_calib_txt" % k], np.uint8).tobytes())
        if ("f%d_plane_txt" % k) in g:
            with open(os.path.join(root, "training/planes/%s.txt" % fid), "wb") as f:
                f.write(np.asarray(g["f%d_plane_txt" % k], np.uint8).tobytes())
    with open(os.path.join(root, "ImageSets/%s.txt" % split), "w") as f:
        f.write("".join(fid + "\n" for fid in FRAME_IDS))
    with open(os.path.join(root, "kitti_infos_%s.pkl" % split), "wb") as f:
        pickle.dump(infos_of(g), f)
    return root


_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(GOLD) as z:
            _gold = {k: z[k] for k in z.files}
    return _gold


# --------------------------------------------------------------------------------------------------------------------- the exact case
def exact_case():
    """-> (calibration dict, (H, W), points (8, 4), expected keep): zeros, ones and powers of two only, small-integer points, so every
    intermediate is exact in any summation order and with or without FMA; exempt from the margin -- its rows sit ON the edges.
    rect = (-y, -z, x + 1); u = (2 r0 + 4 r2) / r2, v = (2 r1 + 2 r2) / r2, depth = (r1 + r2 + 0.5) - 0.5; W = 8, H = 4."""
    calib = {"P2": np.array([[2, 0, 4, 0], [0, 2, 2, 0], [0, 1, 1, 0.5]], F32), "P3": np.zeros((3, 4), F32), "R0": np.eye(3, dtype=F32),
             "Tr_velo2cam": np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 1]], F32)}
    rows = [((1, 4, 0), True),        # r = (-4, 0, 2): u == 0, v = 2                       kept (0 is inside)
            ((1, -4, 0), False),      # r = (4, 0, 2): u == 8 == W                          dropped (W is outside)
            ((1, 0, -1), True),       # r = (0, 1, 2): v == 3 == H - 1                      kept
            ((1, 0, 2), True),        # r = (0, -2, 2): depth == 0, v == 0                  kept
            ((-1, 1, 0), False),      # r = (-1, 0, 0): r_2 == 0, u = -inf                  dropped
            ((-1, 0, 0), False),      # r = (0, 0, 0): 0 / 0 = NaN                          dropped
            ((-3, 0, 0), False),      # r = (0, 0, -2): behind the camera, u = 4, v = 2     dropped by depth = -2
            ((np.nan, 1, 1), False)]  # a NaN row                                           dropped
    pts = np.array([list(p) + [0.25 * i] for i, (p, _) in enumerate(rows)], F32)
    return calib, (4, 8), pts, np.array([k for _, k in rows])
