"""Shared by the occupancy-metrics golden generator and its tests: the golden CASES with their regenerable inputs (integer seeds), and a
numpy restatement of the computation with float64 geometry, written from the description of btc_occ_metrics in
include/btcdet_hip_infer.h -- not from the reference's matrix-inverse formulation.

The restatement is pinned to the golden file (tests/golden/occ_metrics.npz, written by the REAL reference functions) by
tests/test_occ_metrics_cpu.py; the GPU tests then use it as the expectation for seeded cases the golden file does not hold.

Every point of a seeded case lies farther than SAMPLE_MARGIN from every face of every valid box of its scene (violators are resampled, no
case is dropped); the generator asserts that this exceeds max(10 x the reference's float32 deviation, 1e-4 m), which is what lets a GPU
implementation be held to EXACT integers.  Imports nothing that needs a GPU."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "occ_metrics.npz")

N_COUNTERS = 16
SAMPLE_MARGIN = 2e-3                                   # metres
THRESH32 = np.array([np.float32(i * 0.1) for i in range(1, 10)], np.float32)       # the product in double, rounded once
BLOCK_CELLS = 4096                                     # one workgroup's work in the cell pass: 256 threads x 16 cells
MARGIN_EXEMPT = ("on_face",)                           # points exactly ON a face: exact arithmetic instead of a margin


def below(x):
    return np.nextafter(np.float32(x), np.float32(0))


# ------------------------------------------------------------------------------------------------------------------------- inputs
def _cells(rng, shape, half=False, pos_all_extra=3):
    n = int(np.prod(shape))
    cls = rng.rand(n) < 0.6
    pos = cls & (rng.rand(n) < 0.3)
    neg = cls & ~pos
    prob = (rng.rand(n).astype(np.float32) * cls).astype(np.float32)
    if half:                                           # exactly 0.5 and one ulp below, on positive and on other cells
        idx = rng.permutation(n)[:min(n, 24)]
        prob[idx[0::2]] = np.float32(0.5)
        prob[idx[1::2]] = below(0.5)
        cls[idx] = True
        pos[idx[:len(idx) // 2]] = True
        pos[idx[len(idx) // 2:]] = False
        neg = cls & ~pos
    r = lambda a: np.ascontiguousarray(a.reshape(shape))
    return {"batch_pred_occ_prob": r(prob), "general_cls_loss_mask": r(cls.astype(np.uint8)), "pos_mask": r(pos.astype(np.uint8)),
            "neg_mask": r(neg.astype(np.uint8)), "pos_all_num": int(pos.sum()) + (pos_all_extra if pos.sum() else 0)}


def _boxes(rng, B, M, num):
    gt = np.zeros((B, M, 8), np.float32)
    for b in range(B):
        k = num[b]
        gt[b, :k, 0] = rng.uniform(2.0, 68.0, k)
        gt[b, :k, 1] = rng.uniform(-38.0, 38.0, k)
        gt[b, :k, 2] = rng.uniform(-2.0, 0.0, k)
        gt[b, :k, 3] = rng.uniform(3.2, 4.6, k)
        gt[b, :k, 4] = rng.uniform(1.4, 1.9, k)
        gt[b, :k, 5] = rng.uniform(1.3, 1.8, k)
        gt[b, :k, 6] = rng.uniform(-np.pi, np.pi, k)
        gt[b, :k, 7] = 1.0
    return gt


def local64(pts, boxes):
    """(n, 3+) points and (m, 7+) boxes, any float type -> float64 (n, m, 3) box-frame coordinates and (m, 3) half extents"""
    p, g = np.asarray(pts, np.float64), np.asarray(boxes, np.float64)
    d = p[:, None, :3] - g[None, :, :3]
    c, s = np.cos(g[:, 6])[None], np.sin(g[:, 6])[None]
    loc = np.stack([d[..., 0] * c + d[..., 1] * s, d[..., 1] * c - d[..., 0] * s, d[..., 2]], -1)
    return loc, g[:, 3:6] * 0.5


def face_distance(pts, boxes, chunk=4096):
    """(n,) the least distance of each point to a face plane of any box (inf without boxes)"""
    out = np.full((len(pts),), np.inf)
    if len(boxes) == 0:
        return out
    for i in range(0, len(pts), chunk):
        loc, half = local64(pts[i:i + chunk], boxes)
        out[i:i + chunk] = np.abs(np.abs(loc) - half[None]).min(axis=(1, 2))
    return out


def _points(rng, gt, num, per_scene, inside=0.5):
    """per scene `per_scene[b]` points, about `inside` of them inside a valid box; every point farther than SAMPLE_MARGIN from every
    face of every valid box of its scene (resampled until it is); probabilities uniform in [0, 1)"""
    pts, bind = [], []
    for b, n in enumerate(per_scene):
        boxes = gt[b, :num[b]]

        def draw(k):
            p = np.empty((k, 3), np.float32)
            p[:, 0], p[:, 1], p[:, 2] = rng.uniform(0.0, 70.0, k), rng.uniform(-40.0, 40.0, k), rng.uniform(-3.0, 1.0, k)
            if len(boxes):
                into = rng.rand(k) < inside
                j = rng.randint(0, len(boxes), k)
                u = rng.uniform(-0.9, 0.9, (k, 3)) * boxes[j, 3:6] * 0.5
                c, s = np.cos(boxes[j, 6]), np.sin(boxes[j, 6])
                w = np.stack([u[:, 0] * c - u[:, 1] * s + boxes[j, 0], u[:, 0] * s + u[:, 1] * c + boxes[j, 1], u[:, 2] + boxes[j, 2]], -1)
                p[into] = w[into].astype(np.float32)
            return p
        p = draw(n)
        todo = np.arange(n)
        for _ in range(100):
            todo = todo[face_distance(p[todo], boxes) <= SAMPLE_MARGIN]
            if len(todo) == 0:
                break
            p[todo] = draw(len(todo))
        else:
            raise AssertionError("could not place the points of scene %d outside the margin" % b)
        pts.append(np.concatenate([p, rng.rand(n, 1).astype(np.float32)], 1))
        bind.append(np.full((n,), b, np.int64))
    return np.ascontiguousarray(np.concatenate(pts).astype(np.float32)), np.concatenate(bind)


def seeded_case(seed, shape, M, num, pts, half=False, pad_huge=False, inside=0.5):
    """-> batch_dict of numpy arrays and plain values.  shape = (B, nz, ny, nx) of the occupancy grid, M = rows of gt_boxes, num = valid
    boxes per scene, pts = points per scene; pad_huge: the rows past num[b] hold huge boxes that contain every point"""
    rng = np.random.RandomState(seed)
    B = shape[0]
    assert len(num) == B and len(pts) == B and all(k <= M for k in num)
    bd = {"batch_size": B}
    bd.update(_cells(rng, shape, half))
    gt = _boxes(rng, B, M, num)
    if pad_huge:
        for b in range(B):
            gt[b, num[b]:] = np.array([35.0, 0.0, -1.0, 1000.0, 1000.0, 1000.0, 0.3, 1.0], np.float32)
    bd["gt_boxes"], bd["gt_boxes_num"] = gt, [int(k) for k in num]
    if sum(pts) > 0:
        bd["occ_pnts"], bd["added_occ_b_ind"] = _points(rng, gt, num, pts, inside)
    return bd


def _hand(seed, shape, scenes, M=None, half=False):
    """hand-built geometry: scenes = [(boxes (k, 7), points (n, 4))]"""
    rng = np.random.RandomState(seed)
    B = len(scenes)
    assert shape[0] == B
    M = M or max(1, max(len(bx) for bx, _ in scenes))
    bd = {"batch_size": B}
    bd.update(_cells(rng, shape, half))
    gt = np.zeros((B, M, 8), np.float32)
    pts, bind = [], []
    for b, (bx, p) in enumerate(scenes):
        bx = np.asarray(bx, np.float32).reshape(-1, 7)
        gt[b, :len(bx), :7] = bx
        gt[b, :len(bx), 7] = 1.0
        p = np.asarray(p, np.float32).reshape(-1, 4)
        pts.append(p)
        bind.append(np.full((len(p),), b, np.int64))
    bd["gt_boxes"], bd["gt_boxes_num"] = gt, [len(np.asarray(bx).reshape(-1, 7)) for bx, _ in scenes]
    bd["occ_pnts"], bd["added_occ_b_ind"] = np.ascontiguousarray(np.concatenate(pts)), np.concatenate(bind)
    return bd


def _row_of_boxes(k, heading=0.0, dims=(4.0, 2.0, 1.5)):
    """k boxes 16 m apart along x, dyadic centres"""
    return [[8.0 + 16.0 * j, -4.0, -1.0, dims[0], dims[1], dims[2], heading] for j in range(k)]


def _case_sentinel():
    # what PassOccVox hands over when nothing passed the occupancy threshold; the box CONTAINS the origin, the probability is 0
    bd = _hand(31, (1, 3, 5, 7), [([[0.5, 0.25, 0.0, 4.0, 2.0, 1.5, 0.4]], np.zeros((1, 4), np.float32))])
    return bd


def _case_three_overlap():
    boxes = [[20.0, 3.0, -1.0, 4.0, 2.0, 1.5, 0.3], [20.3, 3.2, -0.9, 4.2, 1.8, 1.6, -0.5], [19.8, 2.9, -1.1, 3.8, 1.9, 1.4, 1.2],
             [50.0, -20.0, -1.0, 4.0, 2.0, 1.5, 0.0]]
    return _hand(32, (1, 3, 5, 7), [(boxes, [[20.05, 3.05, -1.0, 0.55], [60.0, 30.0, 0.0, 0.99]])])


def _case_below_and_max():
    # box 0: every point below 0.1; box 1: several points, the maximum (0.83) decides; box 2: no point; scene 1: one box, one point at 0.25
    b0 = _row_of_boxes(3, heading=0.7)
    p0 = [[8.0, -4.0, -1.0, 0.05], [8.3, -4.1, -0.9, 0.0999], [7.9, -3.9, -1.2, 0.0],
          [24.0, -4.0, -1.0, 0.12], [24.2, -4.2, -0.8, 0.83], [23.7, -3.8, -1.1, 0.41], [24.1, -4.0, -1.3, 0.83]]
    return _hand(33, (2, 3, 5, 7), [(b0, p0), (_row_of_boxes(1, heading=-2.0), [[8.1, -4.1, -1.0, 0.25]])])


def _case_thresh_exact():
    # one box per probability: exactly float32(i * 0.1) and one ulp below, i = 1 .. 9
    probs = [THRESH32[i] for i in range(9)] + [below(THRESH32[i]) for i in range(9)]
    boxes = _row_of_boxes(18, heading=0.25)
    return _hand(34, (1, 3, 5, 7), [(boxes, [[bx[0], bx[1], bx[2], p] for bx, p in zip(boxes, probs)])])


def _case_on_face():
    # heading 0 and dyadic coordinates: the arithmetic is exact in float32 on every route.  Box j has ONE point: on each of the six faces,
    # on a corner, and (box 7) one float32 step outside the +x face
    # (centres the reference's float32 matrix inverse reproduces exactly: it does not for every dyadic value, e.g. 56 or 104)
    boxes = [[x, -4.0, -1.0, 4.0, 2.0, 1.5, 0.0] for x in (8.0, 16.0, 24.0, 32.0, 40.0, 48.0, 64.0, 72.0)]
    off = [(2.0, 0.0, 0.0), (-2.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 0.75), (0.0, 0.0, -0.75), (2.0, 1.0, 0.75)]
    pts = [[bx[0] + o[0], bx[1] + o[1], bx[2] + o[2], 0.95] for bx, o in zip(boxes, off)]
    pts.append([np.nextafter(np.float32(boxes[7][0] + 2.0), np.float32(1e9)), -4.0, -1.0, 0.95])
    return _hand(35, (1, 3, 5, 7), [(boxes, pts)])


def _case_points_no_boxes():
    # scene 0: points, no boxes; scene 1: boxes, no points (they still count in box_num_sum); scene 2: both
    bd = seeded_case(36, (3, 3, 5, 7), 5, [0, 4, 3], [20, 0, 30])
    return bd


CASES = {
    "one_cell": lambda: seeded_case(1, (1, 1, 1, 1), 1, [1], [1], inside=1.0),
    "c105_b1": lambda: seeded_case(2, (1, 3, 5, 7), 65, [65], [63]),
    "c105_b2": lambda: seeded_case(3, (2, 3, 5, 7), 65, [65, 40], [64, 65]),
    "block_minus_1": lambda: seeded_case(4, (1, 1, 1, BLOCK_CELLS - 1), 1, [1], [64], inside=0.8),
    "block": lambda: seeded_case(5, (1, 1, 1, BLOCK_CELLS), 1, [1], [65], inside=0.8),
    "block_plus_1": lambda: seeded_case(6, (1, 1, 1, BLOCK_CELLS + 1), 65, [33], [63]),
    "c70001_b8": lambda: seeded_case(7, (8, 1, 1, 8751), 65, [65, 0, 1, 64, 12, 65, 7, 30], [300, 10, 1, 0, 64, 65, 63, 500], half=True),
    "m300": lambda: seeded_case(12, (2, 3, 5, 7), 300, [300, 257], [500, 65]),
    "n80000": lambda: seeded_case(8, (2, 3, 5, 7), 65, [65, 33], [40000, 40000], inside=0.02),
    "cells_half": lambda: seeded_case(9, (1, 3, 5, 7), 1, [1], [1], half=True),
    "huge_padding": lambda: seeded_case(10, (2, 3, 5, 7), 65, [3, 0], [65, 40], pad_huge=True, inside=0.7),
    "points_no_boxes": _case_points_no_boxes,
    "sentinel": _case_sentinel,
    "three_overlap": _case_three_overlap,
    "below_and_max": _case_below_and_max,
    "thresh_exact": _case_thresh_exact,
    "on_face": _case_on_face,
    "no_occ_pnts": lambda: {k: v for k, v in seeded_case(11, (1, 3, 5, 7), 4, [4], [5]).items() if k not in ("occ_pnts", "added_occ_b_ind")},
}
EPOCH = ("c105_b2", "block_plus_1", "below_and_max")      # three consecutive batches of an evaluation run


_INPUTS = {}


def case_inputs(name):
    """the case's batch_dict, built once per process and shared: callers leave it unchanged"""
    if name not in _INPUTS:
        _INPUTS[name] = CASES[name]()
        for v in _INPUTS[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _INPUTS[name]


# ------------------------------------------------------------------------------------------------------------------- restatement
def box_max(bd, slack=0.0, chunk=4096):
    """(B, M) float32: per valid box the highest probability among the scene's points inside it (-1 where none / not a valid box).
    Inside: all three |box-frame coordinates| <= half extent + slack, float64."""
    gt, num = np.asarray(bd["gt_boxes"]), [int(k) for k in bd["gt_boxes_num"]]
    B, M = gt.shape[0], gt.shape[1]
    best = np.full((B, M), -1.0, np.float32)
    if "occ_pnts" not in bd:
        return best
    pts, bind = np.asarray(bd["occ_pnts"]), np.asarray(bd["added_occ_b_ind"]).reshape(-1)
    for b in range(B):
        k = min(max(num[b], 0), M)
        p = pts[bind == b]
        if k == 0 or len(p) == 0:
            continue
        for i in range(0, len(p), chunk):
            q = p[i:i + chunk]
            loc, half = local64(q, gt[b, :k])
            inside = (np.abs(loc) <= half[None] + slack).all(-1)                      # (n, k)
            cand = np.where(inside, q[:, 3:4], np.float32(-1.0)).max(0).astype(np.float32)
            best[b, :k] = np.maximum(best[b, :k], cand)
    return best


def counters(bd, slack=0.0):
    """-> int64 [16]: total, pos_num, neg_num, pos_predict, pos_correct, pos_all_num, box_num_sum, occ_box_num[0..8]"""
    prob = np.asarray(bd["batch_pred_occ_prob"], np.float32).reshape(-1)
    cls, pos, neg = (np.asarray(bd[k]).reshape(-1) != 0 for k in ("general_cls_loss_mask", "pos_mask", "neg_mask"))
    hit = prob >= np.float32(0.5)
    out = np.zeros((N_COUNTERS,), np.int64)
    out[:6] = [cls.sum(), pos.sum(), neg.sum(), hit.sum(), (pos & hit).sum(), int(bd["pos_all_num"])]
    if "gt_boxes" in bd:
        M = np.asarray(bd["gt_boxes"]).shape[1]
        out[6] = sum(min(max(int(k), 0), M) for k in bd["gt_boxes_num"])
        best = box_max(bd, slack)
        for i in range(9):
            out[7 + i] = int((best >= THRESH32[i]).sum())
    return out


def floats(c):
    """precision, recall, f1 as float32, by the float32 operations of the reference's call_precision_recall_f1"""
    f = np.float32
    p = f(c[4]) / max(f(c[3]), f(1.0))
    r = f(c[4]) / max(f(c[1]), f(1.0))
    f1 = f(2.0) * p * r / max(f(p + r), f(1e-8))
    return f(p), f(r), f(f1)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def load_golden():
    return np.load(GOLDEN)
