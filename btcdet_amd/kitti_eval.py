"""KITTI AP evaluation on the GPU: the reference's ``kitti_object_eval_python.eval`` (numba on the CPU plus numba.cuda, neither of which
exists on ROCm) with the overlaps and the matching in HIP (csrc/kitti_eval.hip, include/btcdet_hip_infer.h).

    result_str, ret_dict, pr_rc_details = get_official_eval_result(gt_annos, dt_annos, class_names, coverage_rates=None)

has the reference's signature, keys (``Car_3d/moderate_R40`` ...) and string format; ``eval_class`` returns the reference's
``recall / real_recall / precision / orientation`` arrays of shape [class, difficulty, overlap level, 41].  ``KittiEvaluator`` takes
``BtcPredictor.predict()``'s output batch by batch, builds the detection annotations as ``KittiDataset.generate_prediction_dicts`` does
and evaluates once at the end.

One evaluation is: clean_data's per-box rules vectorised over the concatenated dataset on the host; ONE launch for the overlaps of all
frames and metrics; ONE launch for pass A of every (frame, metric, class, difficulty, level); one read-back; get_thresholds on the host
in float64 (its ``current_recall += 1 / 40`` recurrence is sequential by nature, <= 41 steps per combination); pass B of every
(frame, combination, threshold) in one launch plus a frame-ordered reduction of the AOS similarity; one read-back.  There is no CPU
fallback: without the library every call raises.

The overlap values are exact geometry in float64 (convex clipping).  The reference's rotate_iou.py rounds its boxes to float32 and runs
under numba.cuda; it cannot execute where this project runs, so the values are pinned to geometry (tests/kitti_eval_ref.py), the
matching / threshold / AP logic to an execution of the reference's eval.py (tests/golden/gen_kitti_eval_golden.py).
"""
import numpy as np
import torch

from . import _lib

CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'Truck']
MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
N_SAMPLE_PTS = 41
MAX_PER_FRAME = 1024


# --------------------------------------------------------------------------------------------------------------------- host side
class Dataset(object):
    """the annotations of all frames concatenated (float64), the frame tables of the C ABI, and their device copies"""

    def __init__(self, gt_annos, dt_annos, device=None):
        if len(gt_annos) != len(dt_annos):
            raise ValueError("%d ground-truth frames, %d detection frames" % (len(gt_annos), len(dt_annos)))
        F = self.F = len(gt_annos)
        f64 = np.float64

        def cat(annos, key, width=None):
            parts = [np.asarray(a[key], dtype=f64).reshape((-1,) if width is None else (-1, width)) for a in annos]
            return np.concatenate(parts, 0) if parts else np.zeros((0,) if width is None else (0, width), f64)

        def names(annos):
            parts = [np.asarray(a["name"]).astype(str).reshape(-1) for a in annos]
            return np.concatenate(parts) if parts else np.zeros((0,), dtype=str)

        n_gt = np.array([len(a["name"]) for a in gt_annos], dtype=np.int64)
        n_dt = np.array([len(a["name"]) for a in dt_annos], dtype=np.int64)
        self.gt_name, self.dt_name = names(gt_annos), names(dt_annos)
        self.gt_rows = np.concatenate([cat(gt_annos, "bbox", 4), cat(gt_annos, "location", 3), cat(gt_annos, "dimensions", 3),
                                       cat(gt_annos, "rotation_y")[:, None], cat(gt_annos, "alpha")[:, None]], 1)
        self.dt_rows = np.concatenate([cat(dt_annos, "bbox", 4), cat(dt_annos, "location", 3), cat(dt_annos, "dimensions", 3),
                                       cat(dt_annos, "rotation_y")[:, None], cat(dt_annos, "alpha")[:, None], cat(dt_annos, "score")[:, None]], 1)
        self.occluded, self.truncated = cat(gt_annos, "occluded"), cat(gt_annos, "truncated")
        self.coverage = cat(gt_annos, "coverage_rates") if all("coverage_rates" in a for a in gt_annos) else None
        is_dc = self.gt_name == "DontCare"
        self.dc_boxes = np.ascontiguousarray(self.gt_rows[is_dc, :4])
        gt_frame = np.repeat(np.arange(F), n_gt)
        n_dc = np.bincount(gt_frame[is_dc], minlength=F).astype(np.int64) if F else np.zeros((0,), np.int64)
        frames = np.zeros((F + 1, 3), dtype=np.int64)
        frames[1:, 0], frames[1:, 1], frames[1:, 2] = np.cumsum(n_gt), np.cumsum(n_dt), np.cumsum(n_dc)
        pairs = np.zeros((F + 1, 2), dtype=np.int64)
        pairs[1:, 0], pairs[1:, 1] = np.cumsum(n_dt * n_gt), np.cumsum(n_dt * n_dc)
        if frames.max() >= 2 ** 31:
            raise ValueError("more than 2^31 boxes")
        self.h_frames = np.ascontiguousarray(frames.astype(np.int32))
        self.h_pairs = pairs
        self.NG, self.ND, self.P, self.PD = int(frames[F, 0]), int(frames[F, 1]), int(pairs[F, 0]), int(pairs[F, 1])
        self.alpha0 = next((a["alpha"] for a in dt_annos if np.asarray(a["alpha"]).shape[0] != 0), None)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._dev = None
        self._ov = None

    @property
    def compute_aos(self):
        """the reference's check: the first non-empty detection frame decides"""
        return self.alpha0 is not None and bool(self.alpha0[0] != -10)

    def dev(self):
        if self._dev is None:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
            self._dev = {"gt": up(self.gt_rows), "dt": up(self.dt_rows), "dc": up(self.dc_boxes), "frames": up(self.h_frames),
                         "pairs": up(self.h_pairs)}
        return self._dev

    def overlaps(self, timings=None):
        """-> (ov [3, P], ov_dc [PD]) float64 on the device, computed once"""
        if self._ov is None:
            d = self.dev()
            t = _Stage(timings, "overlaps_ms")
            ov = torch.empty((3, self.P), dtype=torch.float64, device=self.device)
            ov_dc = torch.empty((self.PD,), dtype=torch.float64, device=self.device)
            _lib.check(_lib.lib().btc_kitti_overlaps(_lib.ptr(d["gt"]), _lib.ptr(d["dt"]), _lib.ptr(d["dc"]), _lib.ptr(d["frames"]), _lib.ptr(d["pairs"]),
                                                     _lib.i3p(self.h_frames), self.F, _lib.ptr(ov), _lib.ptr(ov_dc), _lib.stream_ptr()),
                       "btc_kitti_overlaps")
            t.stop()
            self._ov = (ov, ov_dc)
        return self._ov

    def frame_overlaps(self, f):
        """the three [n_dt, n_gt] blocks and the [n_dt, n_dc] block of frame f as numpy arrays (for inspection and tests)"""
        ov, ov_dc = self.overlaps()
        g, d, c = (int(self.h_frames[f + 1, i] - self.h_frames[f, i]) for i in range(3))
        p0, q0 = int(self.h_pairs[f, 0]), int(self.h_pairs[f, 1])
        return ov[:, p0:p0 + d * g].reshape(3, d, g).cpu().numpy(), ov_dc[q0:q0 + d * c].reshape(d, c).cpu().numpy()


class _Stage(object):
    """HIP events around one stage's launches when a timings dict is given (tools/eval_bench.py); nothing otherwise"""

    def __init__(self, timings, key):
        self.timings, self.key = timings, key
        if timings is not None:
            self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.a.record()

    def stop(self):
        if self.timings is not None:
            self.b.record()
            self.b.synchronize()
            self.timings[self.key] = self.a.elapsed_time(self.b)


def clean_data(ds, classes_int, difficultys):
    """clean_data's per-box rules for every (class, difficulty), vectorised over the concatenated dataset
    -> ign_gt [C * D, NG] int8, ign_dt [C * D, ND] int8 (0 counted, 1 ignored, -1 another class), num_valid_gt [C, D]"""
    C, D = len(classes_int), len(difficultys)
    gname, dname = np.char.lower(ds.gt_name) if ds.NG else ds.gt_name, np.char.lower(ds.dt_name) if ds.ND else ds.dt_name
    g_h = ds.gt_rows[:, 3] - ds.gt_rows[:, 1]
    d_h = np.abs(ds.dt_rows[:, 3] - ds.dt_rows[:, 1])
    ign_gt = np.empty((C * D, ds.NG), dtype=np.int8)
    ign_dt = np.empty((C * D, ds.ND), dtype=np.int8)
    for ci, cls in enumerate(classes_int):
        cur = CLASS_NAMES[cls].lower()
        same = gname == cur
        neighbour = (gname == "person_sitting") if cur == "pedestrian" else (gname == "van") if cur == "car" else np.zeros(ds.NG, dtype=bool)
        dsame = dname == cur
        for di, diff in enumerate(difficultys):
            if isinstance(diff, (list, tuple)) and len(diff) == 2:
                if ds.coverage is None:
                    raise KeyError("coverage_rates difficulties need gt_annos[...]['coverage_rates']")
                ignore = (ds.coverage >= diff[0]) & (ds.coverage < diff[1])
                hmin = MIN_HEIGHT[2]
            else:
                ignore = (ds.occluded > MAX_OCCLUSION[diff]) | (ds.truncated > MAX_TRUNCATION[diff]) | (g_h <= MIN_HEIGHT[diff])
                hmin = MIN_HEIGHT[diff]
            ign_gt[ci * D + di] = np.where(same & ~ignore, 0, np.where(neighbour | (same & ignore), 1, -1))
            ign_dt[ci * D + di] = np.where(d_h < hmin, 1, np.where(dsame, 0, -1))
    return ign_gt, ign_dt, (ign_gt == 0).sum(1).reshape(C, D)


def get_thresholds(scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    """the reference's get_thresholds: its loop advances ``current_recall`` at most num_sample_pts times, so the scan between two
    advances is done as one vector comparison of the same float64 expressions"""
    scores = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    n = len(scores)
    if n == 0:
        return []
    idx = np.arange(n, dtype=np.int64)
    l_recall = (idx + 1) / num_gt
    r_recall = (idx + 2) / num_gt
    r_recall[-1] = l_recall[-1]
    current_recall = 0
    out = []
    i = 0
    while i < n:
        skip = (r_recall[i:] - current_recall) < (current_recall - l_recall[i:])
        skip[-1] = False
        i += int(np.argmin(skip))      # the first index that is kept
        out.append(scores[i])
        current_recall += 1 / (num_sample_pts - 1.0)
        i += 1
    return out


def _curves(counts, sim, n_thr, compute_aos):
    """counts [..., 41, 3], sim [..., 41], n_thr [...] -> recall, real_recall, precision, orientation [..., 41] as eval_class fills them"""
    tp, fp, fn = (counts[..., i].astype(np.float64) for i in range(3))
    live = np.arange(N_SAMPLE_PTS) < n_thr[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        rec = np.where(live, tp / (tp + fn), 0.0)
        prec = np.where(live, tp / (tp + fp), 0.0)
        aos = np.where(live, sim / (tp + fp), 0.0) if compute_aos else np.zeros_like(rec)
    real = np.where(live, np.maximum.accumulate(rec, -1), 0.0)
    back = lambda a: np.where(live, np.maximum.accumulate(a[..., ::-1], -1)[..., ::-1], 0.0)  # noqa: E731
    return back(rec), real, back(prec), back(aos) if compute_aos else aos


def evaluate(ds, classes_int, difficultys, min_overlaps, metric_first=0, n_metric=3, compute_aos=False, timings=None):
    """every combination of the metrics metric_first .. metric_first + n_metric - 1 -> {metric: {"recall", "real_recall", "precision",
    "orientation": [C, D, K, 41], "counts": [C, D, K, 41, 3], "n_thresholds": [C, D, K]}}"""
    L = _lib.lib()
    classes_int = [int(c) for c in classes_int]
    min_overlaps = np.ascontiguousarray(np.asarray(min_overlaps, dtype=np.float64))
    K, C, D, M = min_overlaps.shape[0], len(classes_int), len(difficultys), int(n_metric)
    if min_overlaps.shape != (K, 3, C):
        raise ValueError("min_overlaps must be [levels, 3, classes], got %r" % (min_overlaps.shape,))
    combos = M * C * D * K
    ign_gt, ign_dt, n_valid = clean_data(ds, classes_int, difficultys)
    dev, d = ds.device, ds.dev()
    ov, ov_dc = ds.overlaps(timings)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    g_ign_gt, g_ign_dt, g_mo = up(ign_gt), up(ign_dt), up(min_overlaps)
    hf = _lib.i3p(ds.h_frames)
    # pass A: the true positives of every frame and combination
    tp_det = torch.empty((combos, ds.NG), dtype=torch.int32, device=dev)
    tp_count = torch.empty((combos,), dtype=torch.int32, device=dev)
    stage = _Stage(timings, "match_tp_ms")
    _lib.check(L.btc_kitti_match_tp(_lib.ptr(ov), _lib.ptr(d["dt"]), _lib.ptr(g_ign_gt), _lib.ptr(g_ign_dt), _lib.ptr(g_mo), _lib.ptr(d["frames"]),
                                    _lib.ptr(d["pairs"]), hf, ds.F, metric_first, M, C, D, K, _lib.ptr(tp_det), _lib.ptr(tp_count), _lib.stream_ptr()),
               "btc_kitti_match_tp")
    stage.stop()
    h_tp = tp_det.cpu().numpy()      # the one read-back of pass A
    scores = ds.dt_rows[:, 12]
    thr = np.zeros((combos, N_SAMPLE_PTS), dtype=np.float64)
    n_thr = np.zeros((combos,), dtype=np.int32)
    for co in range(combos):
        c, dd = (co // (K * D)) % C, (co // K) % D
        row = h_tp[co]
        t = get_thresholds(scores[row[row >= 0]], int(n_valid[c, dd]))
        n_thr[co] = len(t)
        thr[co, :len(t)] = t
    # pass B: tp / fp / fn / similarity of every frame, combination and threshold
    aos = bool(compute_aos) and metric_first == 0
    counts = torch.empty((combos, N_SAMPLE_PTS, 3), dtype=torch.int32, device=dev)
    sim = torch.empty((C * D * K, N_SAMPLE_PTS), dtype=torch.float64, device=dev)
    ws_bytes = L.btc_kitti_match_stats_ws_bytes(ds.F, C, D, K, int(aos))
    ws = _lib.workspace(ws_bytes, dev)
    g_thr, g_nthr = up(thr), up(n_thr)
    stage = _Stage(timings, "match_stats_ms")
    _lib.check(L.btc_kitti_match_stats(_lib.ptr(ov), _lib.ptr(ov_dc), _lib.ptr(d["gt"]), _lib.ptr(d["dt"]), _lib.ptr(g_ign_gt), _lib.ptr(g_ign_dt),
                                       _lib.ptr(g_mo), _lib.ptr(g_thr), _lib.ptr(g_nthr), _lib.ptr(d["frames"]), _lib.ptr(d["pairs"]), hf, ds.F,
                                       metric_first, M, C, D, K, int(aos), _lib.ptr(counts), _lib.ptr(sim), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()),
               "btc_kitti_match_stats")
    stage.stop()
    h_counts = counts.cpu().numpy().reshape(M, C, D, K, N_SAMPLE_PTS, 3)
    h_sim = sim.cpu().numpy().reshape(C, D, K, N_SAMPLE_PTS)
    n_thr = n_thr.reshape(M, C, D, K)
    out = {}
    for mi in range(M):
        metric = metric_first + mi
        with_aos = aos and metric == 0
        rec, real, prec, ori = _curves(h_counts[mi], h_sim, n_thr[mi], with_aos)
        out[metric] = {"recall": rec, "real_recall": real, "precision": prec, "orientation": ori, "counts": h_counts[mi], "n_thresholds": n_thr[mi]}
    return out


# --------------------------------------------------------------------------------------------------------------------- reference interface
def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, num_parts=100):
    """the reference's eval_class (num_parts is accepted and unused: overlaps are computed within a frame only)"""
    r = evaluate(Dataset(gt_annos, dt_annos), current_classes, difficultys, min_overlaps, int(metric), 1, compute_aos)[int(metric)]
    return {k: r[k] for k in ("recall", "real_recall", "precision", "orientation")}


_R11 = np.arange(0, N_SAMPLE_PTS, 4)      # the 11 recall positions 0, 0.1, ... 1 of the 41-point curve
_R40 = np.arange(1, N_SAMPLE_PTS)         # the 40 positions 1/40 ... 1


def _ap(curve, points):
    """average precision in percent: the mean of the curve [..., 41] at the given sample points"""
    return curve[..., points].sum(axis=-1) * (100.0 / len(points))


def _difficulty_labels(difficultys):
    if isinstance(difficultys[0], int):
        return ["easy", "moderate", "hard"][:len(difficultys)]
    return ["%s<=cvrg<%s" % (lo, hi) for lo, hi in difficultys]


def _pr_details(classes_int, precision, real_recall, difficultys):
    """per class name and difficulty label: the precision / real-recall curves of the FIRST overlap level at the R11 and R40 points"""
    labels = _difficulty_labels(difficultys)
    table = {}
    for j, cls in enumerate(classes_int):
        table[CLASS_NAMES[cls]] = {
            label: {"R11_pc": precision[j, d, 0, _R11], "R11_rc": real_recall[j, d, 0, _R11],
                    "R40_pc": precision[j, d, 0, _R40], "R40_rc": real_recall[j, d, 0, _R40]}
            for d, label in enumerate(labels)}
    return table


_VEHICLE = np.array([name in ("Car", "Van", "Truck") for name in CLASS_NAMES])


def official_min_overlaps(classes_int):
    """[2 levels, 3 metrics, classes]: the official level (vehicles 0.7, the rest 0.5, every metric) and the loose one (bev / 3d:
    0.5 and 0.25; the image box keeps the official level, except Truck at 0.5)"""
    official = np.where(_VEHICLE, 0.7, 0.5)
    table = np.empty((2, 3, len(CLASS_NAMES)))
    table[0] = official
    table[1, 0] = official
    table[1, 0, CLASS_NAMES.index("Truck")] = 0.5
    table[1, 1:] = np.where(_VEHICLE, 0.5, 0.25)
    return table[:, :, classes_int]


def _classes_to_int(current_classes):
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    return [CLASS_NAMES.index(c) if isinstance(c, str) else int(c) for c in current_classes]


def get_official_eval_result(gt_annos, dt_annos, current_classes, coverage_rates=None, PR_detail_dict=None):
    """-> (result_str, ret_dict, pr_rc_details) as the reference; nothing is printed"""
    classes = _classes_to_int(current_classes)
    min_overlaps = official_min_overlaps(classes)
    ds = Dataset(gt_annos, dt_annos)
    compute_aos = ds.compute_aos
    difficultys = [0, 1, 2] if coverage_rates is None else coverage_rates
    per = evaluate(ds, classes, difficultys, min_overlaps, 0, 3, compute_aos)
    bbox, bev, d3 = per[0]["precision"], per[1]["precision"], per[2]["precision"]
    if PR_detail_dict is not None:
        PR_detail_dict["bbox"] = bbox
        if compute_aos:
            PR_detail_dict["aos"] = per[0]["orientation"]
        PR_detail_dict["bev"], PR_detail_dict["3d"] = bev, d3
    pr_rc_details = {"bev": _pr_details(classes, bev, per[1]["real_recall"], difficultys),
                     "3d": _pr_details(classes, d3, per[2]["real_recall"], difficultys)}
    table = {key: (_ap(curve, _R11), _ap(curve, _R40)) for key, curve in (("bbox", bbox), ("bev", bev), ("3d", d3))}
    if compute_aos:
        table["aos"] = (_ap(per[0]["orientation"], _R11), _ap(per[0]["orientation"], _R40))
    result, ret_dict = "", {}
    levels = ("easy", "moderate", "hard")
    for j, cls in enumerate(classes):
        name = CLASS_NAMES[cls]
        for i in range(min_overlaps.shape[0]):
            for r40, tag in ((0, "AP"), (1, "AP_R40")):
                result += "{} {}@{:.2f}, {:.2f}, {:.2f}:\n".format(name, tag, *min_overlaps[i, :, j])
                for label, key in (("bbox", "bbox"), ("bev ", "bev"), ("3d  ", "3d")):
                    v = table[key][r40]
                    result += "{} AP:{:.4f}, {:.4f}, {:.4f}\n".format(label, v[j, 0, i], v[j, 1, i], v[j, 2, i])
                if compute_aos:
                    v = table["aos"][r40]
                    result += "aos  AP:{:.2f}, {:.2f}, {:.2f}\n".format(v[j, 0, i], v[j, 1, i], v[j, 2, i])
            if i == 0:
                if compute_aos:
                    for d, lv in enumerate(levels):
                        ret_dict["%s_aos/%s_R40" % (name, lv)] = table["aos"][1][j, d, 0]
                for key, out_key in (("3d", "3d"), ("bev", "bev"), ("bbox", "image")):
                    for d, lv in enumerate(levels):
                        ret_dict["%s_%s/11R_%s" % (name, out_key, lv)] = table[key][0][j, d, 0]
                for key, out_key in (("3d", "3d"), ("bev", "bev"), ("bbox", "image")):
                    for d, lv in enumerate(levels):
                        ret_dict["%s_%s/%s_R40" % (name, out_key, lv)] = table[key][1][j, d, 0]
    return result, ret_dict, pr_rc_details


# --------------------------------------------------------------------------------------------------------------------- annotations
def boxes3d_lidar_to_kitti_camera(boxes3d_lidar, calib):
    """(N, 7) lidar [x, y, z, dx, dy, dz, heading] (z the centre) -> (N, 7) [x, y, z, l, h, w, ry] in the rectified camera frame (y the
    bottom face), float32; calib: {"P2" [3, 4], "R0" [3, 3], "V2C" [3, 4]}.  The input is not modified."""
    f32 = np.float32
    box = np.asarray(boxes3d_lidar, dtype=f32).reshape(-1, 7)
    to_cam = np.asarray(calib["R0"], dtype=f32) @ np.asarray(calib["V2C"], dtype=f32)      # lidar -> rectified camera, [3, 4]
    out = np.empty_like(box)
    floor = box[:, :3] - box[:, 5:6] * np.array([0, 0, 0.5], dtype=f32)                    # the centre of the bottom face
    out[:, :3] = floor @ to_cam[:, :3].T + to_cam[:, 3]
    out[:, 3], out[:, 4], out[:, 5] = box[:, 3], box[:, 5], box[:, 4]                        # (dx, dy, dz) -> (l, h, w)
    out[:, 6] = -box[:, 6] - f32(np.pi / 2)
    return out


# the eight corners of a camera box in its own frame as multiples of (l / 2, h, w / 2): four on the floor, four on the roof (y points down)
_CORNER_SIGNS = np.array([(sx, sy, sz) for sy in (0, -1) for sx, sz in ((1, 1), (1, -1), (-1, -1), (-1, 1))], dtype=np.float32)


def boxes3d_kitti_camera_to_imageboxes(boxes3d, calib, image_shape=None):
    """(N, 7) camera boxes -> (N, 4) [x1, y1, x2, y2]: the bounding box of the eight projected corners, clipped to the image when its
    shape (height, width) is given"""
    f32 = np.float32
    box = np.asarray(boxes3d, dtype=f32).reshape(-1, 7)
    P2 = np.asarray(calib["P2"], dtype=f32)
    half = box[:, None, 3:6] * np.array([0.5, 1.0, 0.5], dtype=f32) * _CORNER_SIGNS          # [N, 8, 3] offsets before the turn
    c, s = np.cos(box[:, 6])[:, None], np.sin(box[:, 6])[:, None]
    x = box[:, 0:1] + c * half[..., 0] + s * half[..., 2]                                   # rotation_y turns about the camera's y axis
    y = box[:, 1:2] + half[..., 1]
    z = box[:, 2:3] - s * half[..., 0] + c * half[..., 2]
    u = (P2[0, 0] * x + P2[0, 1] * y + P2[0, 2] * z + P2[0, 3]) / z                          # the image point: divided by the depth
    v = (P2[1, 0] * x + P2[1, 1] * y + P2[1, 2] * z + P2[1, 3]) / z
    out = np.stack([u.min(1), v.min(1), u.max(1), v.max(1)], axis=1)
    if image_shape is not None:
        last = np.array([image_shape[1] - 1, image_shape[0] - 1] * 2, dtype=f32)
        out = np.clip(out, 0, last)
    return out


def prediction_anno(pred_dict, calib, image_shape, class_names, frame_id=None):
    """one frame's detection annotation as KittiDataset.generate_prediction_dicts builds it (alpha, truncated, occluded stay zero)"""
    np_ = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)  # noqa: E731
    scores, boxes, labels = np_(pred_dict["pred_scores"]), np_(pred_dict["pred_boxes"]), np_(pred_dict["pred_labels"])
    n = scores.shape[0]
    anno = {"name": np.zeros(n), "truncated": np.zeros(n), "occluded": np.zeros(n), "alpha": np.zeros(n), "bbox": np.zeros([n, 4]),
            "dimensions": np.zeros([n, 3]), "location": np.zeros([n, 3]), "rotation_y": np.zeros(n), "score": np.zeros(n),
            "boxes_lidar": np.zeros([n, 7])}
    if n:
        cam = boxes3d_lidar_to_kitti_camera(boxes[:, :7], calib)
        anno.update(name=np.array(class_names)[labels.astype(np.int64) - 1], bbox=boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=image_shape),
                    dimensions=cam[:, 3:6], location=cam[:, 0:3], rotation_y=cam[:, 6], score=scores, boxes_lidar=boxes)
    anno["frame_id"] = frame_id
    return anno


class KittiEvaluator(object):
    """``ev = KittiEvaluator(gt_annos, class_names)``; per batch ``ev.add(frame_ids, pred_dicts, calibs, image_shapes)`` with
    ``BtcPredictor.predict()``'s pred_dicts; ``ev.result()`` evaluates once.  gt_annos[i] belongs to the i-th frame added; a calibration
    is ``{"P2", "R0", "V2C"}`` (or an object with those attributes, as the reference's Calibration)."""

    def __init__(self, gt_annos, class_names, coverage_rates=None):
        self.gt_annos = list(gt_annos)
        self.class_names = list(class_names)
        self.coverage_rates = coverage_rates
        self.dt_annos = []

    @staticmethod
    def _calib(c):
        return c if isinstance(c, dict) else {"P2": c.P2, "R0": c.R0, "V2C": c.V2C}

    def add(self, frame_ids, pred_dicts, calibs, image_shapes):
        if not (len(frame_ids) == len(pred_dicts) == len(calibs) == len(image_shapes)):
            raise ValueError("add(): one frame id, calibration and image shape per pred_dict")
        for fid, pd, cal, shape in zip(frame_ids, pred_dicts, calibs, image_shapes):
            self.dt_annos.append(prediction_anno(pd, self._calib(cal), shape, self.class_names, fid))
        return self

    def result(self, PR_detail_dict=None):
        if len(self.dt_annos) != len(self.gt_annos):
            raise ValueError("%d frames added, %d ground-truth frames" % (len(self.dt_annos), len(self.gt_annos)))
        return get_official_eval_result(self.gt_annos, self.dt_annos, self.class_names, coverage_rates=self.coverage_rates,
                                        PR_detail_dict=PR_detail_dict)
