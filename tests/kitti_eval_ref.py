"""The KITTI evaluation restated in numpy float64: what btcdet_amd/kitti_eval.py and csrc/kitti_eval.hip are held to.

It restates the reference's kitti_object_eval_python/eval.py (clean_data, the three overlaps, the two passes of compute_statistics_jit,
get_thresholds, eval_class, get_official_eval_result) in our own words, loop by loop where the order of a loop decides a result.  The
rotated intersection is EXACT GEOMETRY: one rectangle is clipped against the four half-planes of the other (Sutherland-Hodgman) in
float64.  The reference's own rotated overlap (rotate_iou.py) is numba.cuda and runs on no machine this project has, so the overlap
VALUES of the project are pinned to this geometry, not to an execution of that kernel; tests/golden/gen_kitti_eval_golden.py runs the
reference's real matching logic on top of these values and tests/test_kitti_eval_cpu.py holds this file to its output.

Also here: the seeded case generator (the golden file stores outputs only) and margins(), the distances that make exact decisions a fair
demand of an implementation whose overlaps carry the project's IoU tolerance (rtol 1e-4 / atol 2e-5).
"""
import math

import numpy as np

CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'Truck']
MIN_HEIGHT = [40, 25, 25]
MAX_OCCLUSION = [0, 1, 2]
MAX_TRUNCATION = [0.15, 0.3, 0.5]
LEVELS = (0.7, 0.5, 0.25)
MARGIN = {"level": 1e-4, "gap": 2e-4, "limit": 1e-6}
N_SAMPLE_PTS = 41


# ------------------------------------------------------------------------------------------------------------------ overlaps
def _corners(b):
    """rotate_iou.py's rbbox_to_corners: (cx, cy, xd, yd, angle) -> 4 corners, clockwise angle"""
    c, s = math.cos(b[4]), math.sin(b[4])
    hx, hy = b[2] / 2, b[3] / 2
    return [(c * x + s * y + b[0], -s * x + c * y + b[1]) for x, y in ((-hx, -hy), (-hx, hy), (hx, hy), (hx, -hy))]


def clip_area(b1, b2):
    """area of the intersection of two rotated rectangles (cx, cy, xd, yd, angle), float64, by convex clipping"""
    dx, dy = b1[0] - b2[0], b1[1] - b2[1]
    r = 0.5 * (math.hypot(b1[2], b1[3]) + math.hypot(b2[2], b2[3]))
    if dx * dx + dy * dy > r * r:      # the circumscribed circles are apart
        return 0.0
    poly = _corners(b1)
    clip = _corners(b2)
    # orientation of the clip polygon: the inside of edge p -> q is the side its own centre lies on
    for k in range(4):
        p, q = clip[k], clip[(k + 1) % 4]
        ex, ey = q[0] - p[0], q[1] - p[1]
        side = ex * (b2[1] - p[1]) - ey * (b2[0] - p[0])
        sign = 1.0 if side >= 0 else -1.0
        out = []
        n = len(poly)
        for i in range(n):
            a, b = poly[i], poly[(i + 1) % n]
            da = sign * (ex * (a[1] - p[1]) - ey * (a[0] - p[0]))
            db = sign * (ex * (b[1] - p[1]) - ey * (b[0] - p[0]))
            if da >= 0:
                out.append(a)
            if (da >= 0) != (db >= 0):
                t = da / (da - db)
                out.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])))
        poly = out
        if len(poly) < 3:
            return 0.0
    s = 0.0
    for i in range(len(poly)):
        a, b = poly[i], poly[(i + 1) % len(poly)]
        s += a[0] * b[1] - a[1] * b[0]
    return abs(s) / 2


def rotate_iou_eval(boxes, qboxes, criterion=-1):
    """rotate_iou_gpu_eval's contract in float64: boxes [N, 5], qboxes [K, 5] -> [N, K]"""
    boxes = np.asarray(boxes, dtype=np.float64)
    qboxes = np.asarray(qboxes, dtype=np.float64)
    out = np.zeros((boxes.shape[0], qboxes.shape[0]), dtype=np.float64)
    bl, ql = boxes.tolist(), qboxes.tolist()
    for i, b in enumerate(bl):
        a1 = b[2] * b[3]
        for j, q in enumerate(ql):
            inter = clip_area(b, q)
            if inter == 0.0:
                continue
            a2 = q[2] * q[3]
            if criterion == -1:
                out[i, j] = inter / (a1 + a2 - inter)
            elif criterion == 0:
                out[i, j] = inter / a1
            elif criterion == 1:
                out[i, j] = inter / a2
            else:
                out[i, j] = inter
    return out


def image_box_overlap(boxes, query, criterion=-1):
    boxes, query = np.asarray(boxes, np.float64).reshape(-1, 4), np.asarray(query, np.float64).reshape(-1, 4)
    iw = np.minimum(boxes[:, None, 2], query[None, :, 2]) - np.maximum(boxes[:, None, 0], query[None, :, 0])
    ih = np.minimum(boxes[:, None, 3], query[None, :, 3]) - np.maximum(boxes[:, None, 1], query[None, :, 1])
    ab = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))[:, None]
    aq = ((query[:, 2] - query[:, 0]) * (query[:, 3] - query[:, 1]))[None, :]
    ok = (iw > 0) & (ih > 0)
    ua = (ab + aq - iw * ih) if criterion == -1 else np.broadcast_to(ab, iw.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, iw * ih / ua, 0.0)


def _bev_rows(a):
    return np.concatenate([a["location"][:, [0, 2]], a["dimensions"][:, [0, 2]], a["rotation_y"][:, None]], 1).astype(np.float64).reshape(-1, 5)


def frame_overlaps(gt, dt):
    """-> ([3][n_dt, n_gt] overlaps of the three metrics, [n_dt, n_dc] detection-against-DontCare overlap)"""
    bbox = image_box_overlap(dt["bbox"], gt["bbox"], -1)
    g, d = _bev_rows(gt), _bev_rows(dt)
    bev = rotate_iou_eval(d, g, -1)
    inter = rotate_iou_eval(d, g, 2)
    gy, gh = gt["location"][:, 1].astype(np.float64), gt["dimensions"][:, 1].astype(np.float64)
    dy, dh = dt["location"][:, 1].astype(np.float64), dt["dimensions"][:, 1].astype(np.float64)
    iw = np.minimum(dy[:, None], gy[None, :]) - np.maximum((dy - dh)[:, None], (gy - gh)[None, :])
    vd = np.prod(dt["dimensions"].astype(np.float64).reshape(-1, 3), 1)[:, None]
    vg = np.prod(gt["dimensions"].astype(np.float64).reshape(-1, 3), 1)[None, :]
    inc = iw * inter
    with np.errstate(divide="ignore", invalid="ignore"):
        d3 = np.where((inter > 0) & (iw > 0), inc / (vd + vg - inc), 0.0)
    dc = gt["bbox"][gt["name"] == "DontCare"].astype(np.float64).reshape(-1, 4)
    return [bbox, bev, d3], image_box_overlap(dt["bbox"], dc, 0)


# ------------------------------------------------------------------------------------------------------------------ clean_data
def clean_data(gt, dt, current_class, difficulty):
    """-> ignored_gt [n_gt], ignored_dt [n_dt] (0 counted, 1 ignored, -1 another class), the number of counted ground truths"""
    cur = CLASS_NAMES[current_class].lower()
    cov = isinstance(difficulty, (list, tuple)) and len(difficulty) == 2
    ign_gt = []
    for i in range(len(gt["name"])):
        name = gt["name"][i].lower()
        height = gt["bbox"][i, 3] - gt["bbox"][i, 1]
        if name == cur:
            valid = 1
        elif (cur == "pedestrian" and name == "person_sitting") or (cur == "car" and name == "van"):
            valid = 0
        else:
            valid = -1
        if cov:
            ignore = difficulty[0] <= gt["coverage_rates"][i] < difficulty[1]
        else:
            ignore = (gt["occluded"][i] > MAX_OCCLUSION[difficulty] or gt["truncated"][i] > MAX_TRUNCATION[difficulty]
                      or height <= MIN_HEIGHT[difficulty])
        if valid == 1 and not ignore:
            ign_gt.append(0)
        elif valid == 0 or (ignore and valid == 1):
            ign_gt.append(1)
        else:
            ign_gt.append(-1)
    ign_dt = []
    hmin = MIN_HEIGHT[2] if cov else MIN_HEIGHT[difficulty]
    for i in range(len(dt["name"])):
        height = abs(dt["bbox"][i, 3] - dt["bbox"][i, 1])
        if height < hmin:
            ign_dt.append(1)
        elif dt["name"][i].lower() == cur:
            ign_dt.append(0)
        else:
            ign_dt.append(-1)
    ign_gt, ign_dt = np.array(ign_gt, dtype=np.int64), np.array(ign_dt, dtype=np.int64)
    return ign_gt, ign_dt, int((ign_gt == 0).sum())


# ------------------------------------------------------------------------------------------------------------------ matching
NO_DETECTION = -10000000


def match(ov, ov_dc, scores, gt_alpha, dt_alpha, ign_gt, ign_dt, metric, min_overlap, thresh=0.0, compute_fp=False, compute_aos=False):
    """one run of the greedy matching -> tp, fp, fn, similarity, the matched true positives' scores"""
    n_dt = len(scores)
    live = [j for j in range(n_dt) if ign_dt[j] != -1 and not (compute_fp and scores[j] < thresh)]
    assigned = set()
    tp = fp = fn = 0
    sim = 0.0
    tp_scores = []
    for i in range(len(ign_gt)):
        if ign_gt[i] == -1:
            continue
        det, valid, best, took_ignored = -1, NO_DETECTION, 0, False
        for j in live:
            if j in assigned:
                continue
            o = ov[j, i]
            if not o > min_overlap:
                continue
            if not compute_fp:
                if scores[j] > valid:
                    det, valid = j, scores[j]
            elif (o > best or took_ignored) and ign_dt[j] == 0:
                best, det, valid, took_ignored = o, j, 1, False
            elif valid == NO_DETECTION and ign_dt[j] == 1:
                det, valid, took_ignored = j, 1, True
        if valid == NO_DETECTION:
            if ign_gt[i] == 0:
                fn += 1
        elif ign_gt[i] == 1 or ign_dt[det] == 1:
            assigned.add(det)
        else:
            tp += 1
            tp_scores.append(scores[det])
            if compute_aos:
                sim += (1.0 + math.cos(gt_alpha[i] - dt_alpha[det])) / 2.0
            assigned.add(det)
    if compute_fp:
        cand = [j for j in live if ign_dt[j] == 0 and j not in assigned]
        fp = len(cand)
        if metric == 0:
            for c in range(ov_dc.shape[1]):
                for j in cand:
                    if j not in assigned and ov_dc[j, c] > min_overlap:
                        assigned.add(j)
                        fp -= 1
    return tp, fp, fn, sim, tp_scores


def get_thresholds(scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    scores = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    current_recall = 0
    out = []
    n = len(scores)
    for i in range(n):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < n - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < n - 1:
            continue
        out.append(scores[i])
        current_recall += 1 / (num_sample_pts - 1.0)
    return out


def curves(pr, compute_aos):
    """pr [n_thresholds, 4] (tp, fp, fn, similarity) -> recall, real_recall, precision, orientation rows of 41"""
    rec, real, prec, aos = (np.zeros(N_SAMPLE_PTS) for _ in range(4))
    n = len(pr)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n):
            rec[i] = pr[i, 0] / (pr[i, 0] + pr[i, 2])
            prec[i] = pr[i, 0] / (pr[i, 0] + pr[i, 1])
            if compute_aos:
                aos[i] = pr[i, 3] / (pr[i, 0] + pr[i, 1])
            real[i] = np.max(rec[:i + 1])
        for i in range(n):
            prec[i] = np.max(prec[i:])
            rec[i] = np.max(rec[i:])
            if compute_aos:
                aos[i] = np.max(aos[i:])
    return rec, real, prec, aos


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, overlaps=None):
    """-> the reference's dict of [class, difficulty, level, 41] arrays, plus "counts": per (class, difficulty, level) the pr table"""
    F = len(gt_annos)
    if overlaps is None:
        overlaps = [frame_overlaps(gt_annos[f], dt_annos[f]) for f in range(F)]
    shape = [len(current_classes), len(difficultys), len(min_overlaps), N_SAMPLE_PTS]
    out = {k: np.zeros(shape) for k in ("recall", "real_recall", "precision", "orientation")}
    counts = {}
    for m, cls in enumerate(current_classes):
        for l, diff in enumerate(difficultys):
            cleaned = [clean_data(gt_annos[f], dt_annos[f], cls, diff) for f in range(F)]
            n_valid = sum(c[2] for c in cleaned)
            for k, mo in enumerate(min_overlaps[:, metric, m]):
                frames = [(overlaps[f][0][metric], overlaps[f][1], dt_annos[f]["score"].astype(np.float64).tolist(),
                           gt_annos[f]["alpha"].astype(np.float64).tolist(), dt_annos[f]["alpha"].astype(np.float64).tolist(),
                           cleaned[f][0].tolist(), cleaned[f][1].tolist()) for f in range(F)]
                tps = []
                for fr in frames:
                    tps += match(*fr, metric, mo)[4]
                thr = get_thresholds(tps, n_valid)
                pr = np.zeros([len(thr), 4])
                for fr in frames:
                    for t, th in enumerate(thr):
                        tp, fp, fn, sim, _ = match(*fr, metric, mo, thresh=th, compute_fp=True, compute_aos=compute_aos)
                        pr[t] += (tp, fp, fn, sim)
                counts[(m, l, k)] = pr
                rec, real, prec, aos = curves(pr, compute_aos)
                out["recall"][m, l, k], out["real_recall"][m, l, k] = rec, real
                out["precision"][m, l, k], out["orientation"][m, l, k] = prec, aos
    out["counts"] = counts
    return out


# ------------------------------------------------------------------------------------------------------------------ the result table
# name -> the overlap levels (official: bbox, bev, 3d; loose: bbox, bev, 3d)
_LEVELS = {"Car": (0.7, 0.7, 0.7, 0.7, 0.5, 0.5), "Pedestrian": (0.5, 0.5, 0.5, 0.5, 0.25, 0.25), "Cyclist": (0.5, 0.5, 0.5, 0.5, 0.25, 0.25),
           "Van": (0.7, 0.7, 0.7, 0.7, 0.5, 0.5), "Person_sitting": (0.5, 0.5, 0.5, 0.5, 0.25, 0.25), "Truck": (0.7, 0.7, 0.7, 0.5, 0.5, 0.5)}


def official_min_overlaps(classes_int):
    """-> [2, 3, classes]"""
    return np.array([_LEVELS[CLASS_NAMES[c]] for c in classes_int]).reshape(-1, 2, 3).transpose(1, 2, 0)


def classes_to_int(current_classes):
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    return [CLASS_NAMES.index(c) if isinstance(c, str) else int(c) for c in current_classes]


def wants_aos(dt_annos):
    for a in dt_annos:
        if a["alpha"].shape[0] != 0:
            return bool(a["alpha"][0] != -10)
    return False


def map11(p):
    return np.sum(p[..., [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40]], axis=-1) / 11 * 100


def map40(p):
    return np.sum(p[..., 1:41], axis=-1) / 40 * 100


def details(classes_int, pc, rc, difficultys):
    if isinstance(difficultys[0], int):
        names = {0: "easy", 1: "moderate", 2: "hard"}
    else:
        names = {i: "{}<=cvrg<{}".format(d[0], d[1]) for i, d in enumerate(difficultys)}
    out = {}
    for j, c in enumerate(classes_int):
        out[CLASS_NAMES[c]] = {names[d]: {"R11_pc": pc[j, d, 0, 0::4], "R11_rc": rc[j, d, 0, 0::4], "R40_pc": pc[j, d, 0, 1:],
                                          "R40_rc": rc[j, d, 0, 1:]} for d in range(pc.shape[1])}
    return out


def format_result(classes_int, min_overlaps, per_metric, compute_aos):
    """per_metric: {0, 1, 2: eval_class dict} -> (result string, ret_dict) as get_official_eval_result writes them"""
    b11, b40 = map11(per_metric[0]["precision"]), map40(per_metric[0]["precision"])
    v11, v40 = map11(per_metric[1]["precision"]), map40(per_metric[1]["precision"])
    d11, d40 = map11(per_metric[2]["precision"]), map40(per_metric[2]["precision"])
    a11 = a40 = None
    if compute_aos:
        a11, a40 = map11(per_metric[0]["orientation"]), map40(per_metric[0]["orientation"])
    res, ret = "", {}
    for j, c in enumerate(classes_int):
        n = CLASS_NAMES[c]
        for i in range(min_overlaps.shape[0]):
            for tag, bb, bv, d3, ao in (("AP", b11, v11, d11, a11), ("AP_R40", b40, v40, d40, a40)):
                res += "%s %s@%.2f, %.2f, %.2f:\n" % ((n, tag) + tuple(min_overlaps[i, :, j]))
                res += "bbox AP:%.4f, %.4f, %.4f\n" % tuple(bb[j, :3, i])
                res += "bev  AP:%.4f, %.4f, %.4f\n" % tuple(bv[j, :3, i])
                res += "3d   AP:%.4f, %.4f, %.4f\n" % tuple(d3[j, :3, i])
                if compute_aos:
                    res += "aos  AP:%.2f, %.2f, %.2f\n" % tuple(ao[j, :3, i])
            if i == 0:
                if compute_aos:
                    for d, dn in enumerate(("easy", "moderate", "hard")):
                        ret["%s_aos/%s_R40" % (n, dn)] = a40[j, d, 0]
                for key, arr in (("3d", d11), ("bev", v11), ("image", b11)):
                    for d, dn in enumerate(("easy", "moderate", "hard")):
                        ret["%s_%s/11R_%s" % (n, key, dn)] = arr[j, d, 0]
                for key, arr in (("3d", d40), ("bev", v40), ("image", b40)):
                    for d, dn in enumerate(("easy", "moderate", "hard")):
                        ret["%s_%s/%s_R40" % (n, key, dn)] = arr[j, d, 0]
    return res, ret


def get_official_eval_result(gt_annos, dt_annos, current_classes, coverage_rates=None, PR_detail_dict=None, per_metric_out=None):
    classes_int = classes_to_int(current_classes)
    mo = official_min_overlaps(classes_int)
    aos = wants_aos(dt_annos)
    diffs = [0, 1, 2] if coverage_rates is None else coverage_rates
    overlaps = [frame_overlaps(g, d) for g, d in zip(gt_annos, dt_annos)]
    per = {m: eval_class(gt_annos, dt_annos, classes_int, diffs, m, mo, aos and m == 0, overlaps) for m in range(3)}
    if per_metric_out is not None:
        per_metric_out.update(per)
    if PR_detail_dict is not None:
        PR_detail_dict["bbox"] = per[0]["precision"]
        if aos:
            PR_detail_dict["aos"] = per[0]["orientation"]
        PR_detail_dict["bev"], PR_detail_dict["3d"] = per[1]["precision"], per[2]["precision"]
    prd = {"bev": details(classes_int, per[1]["precision"], per[1]["real_recall"], diffs),
           "3d": details(classes_int, per[2]["precision"], per[2]["real_recall"], diffs)}
    res, ret = format_result(classes_int, mo, per, aos)
    return res, ret, prd


# ------------------------------------------------------------------------------------------------------------------ seeded cases
_DIMS = {"Car": (3.9, 1.56, 1.6), "Van": (5.0, 2.2, 1.9), "Pedestrian": (0.8, 1.75, 0.65), "Person_sitting": (0.8, 1.3, 0.6),
         "Cyclist": (1.76, 1.73, 0.6), "Truck": (10.0, 3.2, 2.6)}   # (l, h, w)
COVERAGE_RATES = [[0.0, 0.3], [0.3, 0.7], [0.7, 1.01]]


def _away(rng, lo, hi, limits, eps=1e-3):
    while True:
        v = float(rng.uniform(lo, hi))
        if all(abs(v - x) > eps for x in limits):
            return v


def _gt_row(rng, name):
    row = {"name": name, "occluded": float((0, 0, 0, 1, 1, 2, 3)[int(rng.integers(7))]),
           "truncated": _away(rng, 0, 0.6, MAX_TRUNCATION) if rng.random() < 0.3 else 0.0,
           "alpha": float(rng.uniform(-np.pi, np.pi)), "coverage": _away(rng, 0, 1, (0.0, 0.3, 0.7, 1.01))}
    h = _away(rng, 15, 130, MIN_HEIGHT)
    x1, y1 = float(rng.uniform(0, 1100)), float(rng.uniform(100, 240))
    row["bbox"] = [x1, y1, x1 + h * float(rng.uniform(0.4, 2.0)), y1 + h]
    if name == "DontCare":
        row.update(loc=[-1000.0, -1000.0, -1000.0], dims=[-1.0, -1.0, -1.0], ry=-10.0, occluded=-1.0, truncated=-1.0, alpha=-10.0)
        return row
    l, hh, w = (d * float(rng.uniform(0.85, 1.15)) for d in _DIMS[name])
    row.update(loc=[float(rng.uniform(-20, 20)), float(rng.uniform(1.2, 2.0)), float(rng.uniform(5, 60))], dims=[l, hh, w],
               ry=float(rng.uniform(-np.pi, np.pi)))
    return row


def _dt_from(rng, g, det_names, tight, found=True, swap=0.05):
    s = 0.25 if tight else 1.0
    name = g["name"] if g["name"] in det_names else det_names[int(rng.integers(len(det_names)))]
    if rng.random() < swap:
        name = det_names[int(rng.integers(len(det_names)))]
    jit = float(rng.uniform(0.5, 6)) * s
    return {"name": name, "bbox": [g["bbox"][0] + float(rng.normal(0, jit)), g["bbox"][1] + float(rng.normal(0, jit)),
                                   g["bbox"][2] + float(rng.normal(0, jit)), g["bbox"][3] + float(rng.normal(0, jit))],
            "loc": [g["loc"][0] + float(rng.normal(0, 0.12 * s)), g["loc"][1] + float(rng.normal(0, 0.04)), g["loc"][2] + float(rng.normal(0, 0.15 * s))],
            "dims": [d * float(rng.uniform(1 - 0.07 * s, 1 + 0.07 * s)) for d in g["dims"]], "ry": g["ry"] + float(rng.normal(0, 0.08 * s)),
            "alpha": g["alpha"] + float(rng.normal(0, 0.3)), "score": float(rng.uniform(0.4, 1.0) if found else rng.uniform(0.05, 0.7))}


def _frame(rng, max_gt, max_dt, gt_names, det_names, n_gt=None, n_dt=None, pad_real=0.6, found=0.85):
    """ground truths; detections: most ground truths found once (tightly or loosely), a few twice, some detections inside DontCare
    regions, false positives elsewhere; in shuffled order"""
    n_gt = int(rng.integers(0, max_gt + 1)) if n_gt is None else n_gt
    gts = [_gt_row(rng, gt_names[int(rng.integers(len(gt_names)))]) for _ in range(n_gt)]
    dts = []
    for g in gts:
        if g["name"] == "DontCare":
            if rng.random() < 0.6:      # a detection inside a DontCare region
                d = _dt_from(rng, _gt_row(rng, det_names[int(rng.integers(len(det_names)))]), det_names, True, False)
                bw, bh = g["bbox"][2] - g["bbox"][0], g["bbox"][3] - g["bbox"][1]
                d["bbox"] = [g["bbox"][0] + 0.1 * bw, g["bbox"][1] + 0.05 * bh, g["bbox"][0] + 0.8 * bw, g["bbox"][1] + 0.9 * bh]
                dts.append(d)
            continue
        if rng.random() < found:
            dts.append(_dt_from(rng, g, det_names, rng.random() < 0.7 or found >= 1.0, swap=0.05 if found < 1.0 else 0.0))
            if rng.random() < 0.12:
                dts.append(_dt_from(rng, g, det_names, rng.random() < 0.5))
    n_fp = int(rng.integers(0, 4))
    for _ in range(n_fp):
        dts.append(_dt_from(rng, _gt_row(rng, det_names[int(rng.integers(len(det_names)))]), det_names, False, False))
    want = n_dt if n_dt is not None else min(len(dts), max_dt)
    real = [g for g in gts if g["name"] != "DontCare"]
    while len(dts) < want:
        if real and rng.random() < pad_real:
            dts.append(_dt_from(rng, real[int(rng.integers(len(real)))], det_names, rng.random() < 0.5))
        else:
            dts.append(_dt_from(rng, _gt_row(rng, det_names[int(rng.integers(len(det_names)))]), det_names, False, False))
    order = rng.permutation(len(dts))[:want]
    return gts, [dts[i] for i in order]


def _annos(gts, dts, scores, alpha_valid):
    f = np.float64
    gt = {"name": np.array([g["name"] for g in gts], dtype="<U16"), "truncated": np.array([g["truncated"] for g in gts], f),
          "occluded": np.array([g["occluded"] for g in gts], f), "alpha": np.array([g["alpha"] for g in gts], f),
          "bbox": np.array([g["bbox"] for g in gts], f).reshape(-1, 4), "dimensions": np.array([g["dims"] for g in gts], f).reshape(-1, 3),
          "location": np.array([g["loc"] for g in gts], f).reshape(-1, 3), "rotation_y": np.array([g["ry"] for g in gts], f),
          "coverage_rates": np.array([g["coverage"] for g in gts], f)}
    n = len(dts)
    dt = {"name": np.array([d["name"] for d in dts], dtype="<U16"), "truncated": np.zeros(n), "occluded": np.zeros(n),
          "alpha": np.array([d["alpha"] for d in dts], f) if alpha_valid else np.full(n, -10.0),
          "bbox": np.array([d["bbox"] for d in dts], f).reshape(-1, 4), "dimensions": np.array([d["dims"] for d in dts], f).reshape(-1, 3),
          "location": np.array([d["loc"] for d in dts], f).reshape(-1, 3), "rotation_y": np.array([d["ry"] for d in dts], f),
          "score": np.asarray(scores, f)}
    return gt, dt


def frame_margins(gt, dt, ov=None):
    """worst distances of one frame: {"level", "gap", "limit"} (see MARGIN)"""
    (bbox, bev, d3), dc = frame_overlaps(gt, dt) if ov is None else ov
    worst = {"level": np.inf, "gap": np.inf, "limit": np.inf}
    for o in (bbox, bev, d3, dc):
        if o.size:
            worst["level"] = min(worst["level"], float(np.min(np.abs(o[..., None] - np.array(LEVELS)))))
    for o in (bbox, bev, d3):
        for i in range(o.shape[1]):
            c = np.sort(o[:, i][o[:, i] > min(LEVELS) - 1e-3])
            if len(c) > 1:
                worst["gap"] = min(worst["gap"], float(np.min(np.diff(c))))
    lim = []
    if len(gt["name"]):
        hg = gt["bbox"][:, 3] - gt["bbox"][:, 1]
        lim += [np.abs(hg[:, None] - np.array(MIN_HEIGHT, float)), np.abs(gt["truncated"][:, None] - np.array(MAX_TRUNCATION)),
                np.abs(gt["coverage_rates"][:, None] - np.array(sorted({x for p in COVERAGE_RATES for x in p})))]
    if len(dt["name"]):
        lim.append(np.abs(np.abs(dt["bbox"][:, 3] - dt["bbox"][:, 1])[:, None] - np.array(MIN_HEIGHT, float)))
    for a in lim:
        worst["limit"] = min(worst["limit"], float(a.min()))
    return worst


def margins(gt_annos, dt_annos):
    worst = {"level": np.inf, "gap": np.inf, "limit": np.inf}
    for g, d in zip(gt_annos, dt_annos):
        w = frame_margins(g, d)
        worst = {k: min(worst[k], w[k]) for k in worst}
    return worst


def margins_ok(w):
    return w["level"] >= MARGIN["level"] and w["gap"] >= MARGIN["gap"] and w["limit"] >= MARGIN["limit"]


GT_NAMES_FULL = ["Car", "Car", "Car", "Pedestrian", "Pedestrian", "Cyclist", "Van", "Person_sitting", "DontCare", "Truck"]


def make_case(seed, n_frames=100, max_gt=12, max_dt=20, gt_names=GT_NAMES_FULL, det_names=("Car", "Pedestrian", "Cyclist"), tied=False,
              alpha_valid=True, sizes=None, empty_every=0, pad_real=0.6, found=0.85):
    """-> gt_annos, dt_annos.  A frame that violates the margins is drawn again with the next attempt number, so the case is a
    function of its arguments alone.  sizes: per-frame (n_gt, n_dt) or None; empty_every: every k-th frame has no boxes at all; found: the
    share of ground truths with a detection of their own (1.0: every one, tightly: recall reaches 1 and a threshold list its 41 entries)"""
    gt_annos, dt_annos = [], []
    for f in range(n_frames):
        for attempt in range(200):
            rng = np.random.default_rng([seed, f, attempt])
            ng, nd = sizes[f] if sizes is not None else (None, None)
            if empty_every and f % empty_every == 0:
                ng, nd = 0, 0
            gts, dts = _frame(rng, max_gt, max_dt, list(gt_names), list(det_names), ng, nd, pad_real, found)
            scores = rng.integers(1, 10, len(dts)) / 10.0 if tied else np.array([d["score"] for d in dts])
            gt, dt = _annos(gts, dts, scores, alpha_valid)
            if margins_ok(frame_margins(gt, dt)):
                break
        else:
            raise RuntimeError("no frame within the margins after 200 attempts (seed %d, frame %d)" % (seed, f))
        gt_annos.append(gt)
        dt_annos.append(dt)
    return gt_annos, dt_annos


# the cases of tests/golden/kitti_eval.npz: name -> (make_case arguments, classes, coverage_rates)
GOLDEN_CASES = {
    "three": (dict(seed=11, n_frames=100), ["Car", "Pedestrian", "Cyclist"], None),
    "car": (dict(seed=12, n_frames=60), ["Car"], None),
    "no_gt": (dict(seed=13, n_frames=40, gt_names=["Car", "Van", "Pedestrian", "DontCare"]), ["Car", "Cyclist"], None),
    "coverage": (dict(seed=14, n_frames=60), ["Car", "Pedestrian", "Cyclist"], COVERAGE_RATES),
    "no_aos": (dict(seed=15, n_frames=40, alpha_valid=False), ["Car", "Pedestrian"], None),
    "tied": (dict(seed=16, n_frames=60, tied=True), ["Car", "Pedestrian", "Cyclist"], None),
}


_cache = {}


def load_golden():
    """-> (the npz of tests/golden/kitti_eval.npz, its meta dict), read once"""
    import json
    import os
    if "golden" not in _cache:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_eval.npz"))
        _cache["golden"] = (z, json.loads(bytes(z["meta"]).decode()))
    return _cache["golden"]


def cached_case(name, classes=None, coverage_rates=None, **kw):
    """a golden case by name, or make_case(**kw) under `name`: (gt, dt, classes, coverage_rates, {metric: eval_class dict},
    (result, ret_dict, details)) with the restatement's result, computed once per process and shared by the tests"""
    if name not in _cache:
        if name in GOLDEN_CASES:
            kw, classes, coverage_rates = GOLDEN_CASES[name]
        gt, dt = make_case(**kw)
        per = {}
        res = get_official_eval_result(gt, dt, classes, coverage_rates=coverage_rates, per_metric_out=per)
        _cache[name] = (gt, dt, classes, coverage_rates, per, res)
    return _cache[name]


# ------------------------------------------------------------------------------------------------------------------ calibration
def make_calib(seed):
    """a KITTI-like calibration: P2 [3, 4], R0 [3, 3], V2C [3, 4], float32"""
    rng = np.random.default_rng([seed, 77])
    P2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]], dtype=np.float32)
    P2[0, 2] += np.float32(rng.uniform(-5, 5))
    a = rng.normal(0, 0.01, 3)
    R0 = np.array([[1, -a[2], a[1]], [a[2], 1, -a[0]], [-a[1], a[0], 1]], dtype=np.float32)
    V2C = np.array([[7.5e-3, -0.99997, -6.2e-4, -4.07e-3], [1.48e-2, 7.28e-4, -0.99989, -7.63e-2], [0.99986, 7.5e-3, 1.48e-2, -0.2718]],
                   dtype=np.float32)
    return {"P2": P2, "R0": R0, "V2C": V2C}


def make_lidar_boxes(seed, n):
    rng = np.random.default_rng([seed, 78])
    b = np.stack([rng.uniform(4, 60, n), rng.uniform(-20, 20, n), rng.uniform(-1.5, 0.0, n), rng.uniform(0.6, 4.5, n),
                  rng.uniform(0.5, 2.0, n), rng.uniform(1.3, 2.0, n), rng.uniform(-np.pi, np.pi, n)], 1)
    return b.astype(np.float32)
