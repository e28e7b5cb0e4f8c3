"""numpy restatement of include/btcdet_hip_heads.h, ONE np.float32 operation per rounded step, plus the helpers the anchor-target tests
share: the configurations of tests/golden/anchor_targets.npz, the margin checks on inputs, seeded boxes.  Imports nothing that needs a
GPU.

  restate_assign(anchors, slot_cfg, matched, unmatched, class_cfg, gt) -> labels (B, A) i32, targets (B, A, 7) f32, weights (B, A) f32,
                                                                         best (B, A) i32 (the matched row, -1 without an offered box)
  restate_decode(box_preds, anchors, dir_cls_preds, off, lim, bins)    -> boxes (B, A, 7) f32
`recip` chooses the form of val / period: True multiplies by the float32 reciprocal (the header's form), False divides (the reference
run on a CPU).  The margins `margins_assign` / `margins_decode` assert make both decide alike."""
import json
import os

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "anchor_targets.npz")
PI = F(np.pi)
QUARTER_PI = F(np.pi / 4)
TRANSCENDENTAL = (3, 4, 5)       # target / box columns that go through log / exp: compared at rtol 1e-5, atol 1e-6
EXACT = (0, 1, 2, 6)


class ED(dict):
    """attribute dict, as the config loader's"""
    __getattr__ = dict.get
    __setattr__ = dict.__setitem__

    def __init__(self, d=None, **kw):
        super().__init__()
        for k, v in dict(d or {}, **kw).items():
            self[k] = ED(v) if isinstance(v, dict) else ([ED(x) if isinstance(x, dict) else x for x in v] if isinstance(v, list) else v)


# ------------------------------------------------------------------------------------------------------------------- configurations
# spacing 2.0 in x and y and anchors at even coordinates: midpoints, half sizes and overlaps of the `one` map are exact in float32
def _gen(name, size, bottom, matched, unmatched, rots=(0, 1.57)):
    return dict(class_name=name, anchor_sizes=[list(size)], anchor_rotations=list(rots), anchor_bottom_heights=[bottom], align_center=False,
                feature_map_stride=8, matched_threshold=matched, unmatched_threshold=unmatched)


MAPS = {
    # 16 x 16 locations, one configuration with two rotations, sizes that halve exactly
    "one": dict(grid_size=[128, 128, 40], point_cloud_range=[0.0, -15.0, -3.0, 30.0, 15.0, 1.0], class_names=["Car"],
                generator=[_gen("Car", (4.0, 1.5, 1.5), -1.75, 0.6, 0.45)]),
    # 15 x 17 locations, the three KITTI configurations of OpenPCDet on one map; class 4 (Van) has no configuration
    "three": dict(grid_size=[136, 120, 40], point_cloud_range=[0.0, -14.0, -3.0, 32.0, 14.0, 1.0], class_names=["Car", "Pedestrian", "Cyclist", "Van"],
                  generator=[_gen("Car", (3.9, 1.6, 1.56), -1.78, 0.6, 0.45), _gen("Pedestrian", (0.8, 0.6, 1.73), -0.6, 0.5, 0.35),
                             _gen("Cyclist", (1.76, 0.6, 1.73), -0.6, 0.5, 0.35)]),
}


def head_cfg(map_name, matched=None, unmatched=None, device=None, **extra):
    """the DENSE_HEAD configuration of a map; matched / unmatched: per-configuration overrides"""
    m = MAPS[map_name]
    gen = [dict(g) for g in m["generator"]]
    for i, g in enumerate(gen):
        if matched is not None and matched[i] is not None:
            g["matched_threshold"] = float(matched[i])
        if unmatched is not None and unmatched[i] is not None:
            g["unmatched_threshold"] = float(unmatched[i])
    tgt = dict(NAME="AxisAlignedTargetAssigner", POS_FRACTION=-1.0, SAMPLE_SIZE=512, NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False,
               BOX_CODER="ResidualCoder")
    if device is not None:
        tgt["DEVICE"] = device
    cfg = dict(CLASS_AGNOSTIC=False, USE_DIRECTION_CLASSIFIER=True, DIR_OFFSET=0.78539, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2,
               ANCHOR_GENERATOR_CONFIG=gen, TARGET_ASSIGNER_CONFIG=tgt,
               LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2, code_weights=[1.0] * 7)))
    cfg.update(extra)
    return ED(cfg)


def host_tables(cfg, class_names):
    """slot_cfg, matched, unmatched, class_cfg of a configuration, written out independently of btcdet_amd.anchor_targets"""
    gen = cfg.ANCHOR_GENERATOR_CONFIG
    slot_cfg = []
    for i, g in enumerate(gen):
        slot_cfg += [i] * (len(g["anchor_sizes"]) * len(g["anchor_rotations"]))
    names = [g["class_name"] for g in gen]
    class_cfg = []
    for c in range(len(class_names) + 1):
        name = class_names[c - 1]                   # c = 0 -> the last name
        class_cfg.append(names.index(name) if name in names else -1)
    return (np.array(slot_cfg, np.int32), np.array([g["matched_threshold"] for g in gen], F), np.array([g["unmatched_threshold"] for g in gen], F),
            np.array(class_cfg, np.int32))


def gold():
    g = np.load(GOLD)
    return g, json.loads(str(g["cases"]))


# ----------------------------------------------------------------------------------------------------- include/btcdet_hip_heads.h
def limit_period(v, offset, period, recip=True):
    v, period = np.asarray(v, F), F(period)
    q = v * (F(1.0) / period) if recip else v / period
    return v - np.floor(q + F(offset)) * period


def footprint(b, recip=True):
    """(n, >= 7) boxes -> x0, y0, x1, y1, area"""
    b = np.asarray(b, F)
    snapped = np.abs(limit_period(b[:, 6], 0.5, PI, recip)) < QUARTER_PI
    wx, wy = np.where(snapped, b[:, 3], b[:, 4]), np.where(snapped, b[:, 4], b[:, 3])
    hx, hy = wx / F(2), wy / F(2)
    x0, y0, x1, y1 = b[:, 0] - hx, b[:, 1] - hy, b[:, 0] + hx, b[:, 1] + hy
    return x0, y0, x1, y1, (x1 - x0) * (y1 - y0)


def overlaps(anchors, boxes, recip=True):
    """(A, G) float32 nearest-BEV overlaps"""
    ax0, ay0, ax1, ay1, aa = (v[:, None] for v in footprint(anchors, recip))
    gx0, gy0, gx1, gy1, ga = (v[None, :] for v in footprint(boxes, recip))
    w = np.maximum(np.minimum(ax1, gx1) - np.maximum(ax0, gx0), F(0))
    h = np.maximum(np.minimum(ay1, gy1) - np.maximum(ay0, gy0), F(0))
    inter = w * h
    return (inter / np.maximum((aa + ga) - inter, F(1e-6))).astype(F)


def scene_rows(gt_scene):
    """n_b of the header: trailing padding trimmed, row 0 kept"""
    g = np.asarray(gt_scene, F)
    if g.shape[0] == 0:
        return 0
    s = g[:, 0]
    for k in range(1, 7):
        s = s + g[:, k]
    nz = np.flatnonzero(s != 0)
    return max(1, int(nz[-1]) + 1) if nz.size else 1


def encode(g, a):
    """ResidualCoder.encode_torch of box rows g against anchor rows a, both (n, >= 7)"""
    a, g = np.asarray(a, F), np.asarray(g, F)
    dxa, dya, dza = (np.maximum(a[:, k], F(1e-5)) for k in (3, 4, 5))
    dxg, dyg, dzg = (np.maximum(g[:, k], F(1e-5)) for k in (3, 4, 5))
    diag = np.sqrt(dxa * dxa + dya * dya)
    return np.stack([(g[:, 0] - a[:, 0]) / diag, (g[:, 1] - a[:, 1]) / diag, (g[:, 2] - a[:, 2]) / dza, np.log(dxg / dxa), np.log(dyg / dya),
                     np.log(dzg / dza), g[:, 6] - a[:, 6]], axis=1).astype(F)


def restate_assign(anchors, slot_cfg, matched, unmatched, class_cfg, gt, recip=True, details=False):
    anchors, gt = np.asarray(anchors, F), np.asarray(gt, F)
    slot_cfg, class_cfg = np.asarray(slot_cfg, np.int64), np.asarray(class_cfg, np.int64)
    matched, unmatched = np.asarray(matched, F), np.asarray(unmatched, F)
    A, B, slots, num_class = anchors.shape[0], gt.shape[0], slot_cfg.shape[0], class_cfg.shape[0] - 1
    assert A % slots == 0
    mine = slot_cfg[np.arange(A) % slots]
    labels, targets = np.zeros((B, A), np.int32), np.zeros((B, A, 7), F)
    best_row, best_iou, forced_all = -np.ones((B, A), np.int32), np.zeros((B, A), F), np.zeros((B, A), bool)
    for b in range(B):
        n = scene_rows(gt[b])
        rows = gt[b, :n]
        cls = rows[:, 7].astype(np.int32) if n else np.zeros((0,), np.int32)       # truncation
        cfg = np.where((cls >= 0) & (cls <= num_class), class_cfg[np.clip(cls, 0, num_class)], -1) if n else np.zeros((0,), np.int64)
        if n == 0 or A == 0:
            continue
        iou = overlaps(anchors, rows, recip)
        offered = (cfg[None, :] == mine[:, None]) & (cfg[None, :] >= 0)
        top = np.where(offered, iou, F(0)).max(axis=0)                            # over the anchors of the box's configuration
        masked = np.where(offered, iou, F(-1))
        j = masked.argmax(axis=1)                                                  # the smallest index among equal overlaps
        has = offered.any(axis=1)
        best = masked[np.arange(A), j]
        forced = (offered & (iou == top[None, :]) & (top[None, :] > 0)).any(axis=1)
        own = cls[j]
        lab = np.where(forced, own, np.where(best < unmatched[mine], 0, np.where(best >= matched[mine], own, -1)))
        lab = np.where(has, lab, 0).astype(np.int32)
        labels[b] = lab
        fg = lab > 0
        targets[b, fg] = encode(rows[j[fg]], anchors[fg])
        best_row[b] = np.where(has, j, -1)
        best_iou[b], forced_all[b] = np.where(has, best, F(0)), forced & has
    weights = (labels > 0).astype(F)
    if details:
        return labels, targets, weights, best_row, best_iou, forced_all
    return labels, targets, weights, best_row


def restate_decode(box_preds, anchors, dir_cls_preds, off=0.0, lim=0.0, bins=0, recip=True):
    t, a = np.asarray(box_preds, F), np.asarray(anchors, F)[None]
    diag = np.sqrt(a[..., 3] * a[..., 3] + a[..., 4] * a[..., 4])
    out = np.empty(t.shape, F)
    out[..., 0] = t[..., 0] * diag + a[..., 0]
    out[..., 1] = t[..., 1] * diag + a[..., 1]
    out[..., 2] = t[..., 2] * a[..., 5] + a[..., 2]
    for k in (3, 4, 5):
        out[..., k] = np.exp(t[..., k]) * a[..., k]
    rot = t[..., 6] + a[..., 6]
    if dir_cls_preds is not None:
        period = F(2 * np.pi / bins)
        k = np.asarray(dir_cls_preds, F).argmax(axis=-1)                           # the smallest index of the largest logit
        lp = limit_period(rot - F(off), lim, period, recip)
        rot = (lp + F(off)) + period * k.astype(F)
    out[..., 6] = rot
    return out


# ------------------------------------------------------------------------------------------------- head.npz at KITTI size
def kitti_head():
    """the KITTI-Car head of tests/golden/head.npz: (cfg, class_names, flat anchors (70 400, 7), gt)"""
    from btcdet_amd.dense_head import make_anchors
    cfg = head_cfg("one")
    cfg.ANCHOR_GENERATOR_CONFIG = [ED(class_name="Car", anchor_sizes=[[3.9, 1.6, 1.56]], anchor_rotations=[0, 1.57], anchor_bottom_heights=[-1.78],
                                         align_center=False, feature_map_stride=8, matched_threshold=0.6, unmatched_threshold=0.45)]
    anchors = make_anchors(np.array([0, -40, -3, 70.4, 40, 1], np.float32), cfg.ANCHOR_GENERATOR_CONFIG, np.array([1408, 1600, 40]), "cpu")[0]
    g = np.load(os.path.join(HERE, "golden", "head.npz"))
    return cfg, ["Car"], anchors, g


def check_against_head_npz(labels, targets, weights, g):
    assert np.array_equal(labels.astype(np.int8), g["box_cls_labels"])
    rows = np.stack(np.nonzero(np.abs(targets).sum(-1)), 1).astype(np.int32)
    assert np.array_equal(rows, g["reg_rows"])
    vals = targets[rows[:, 0], rows[:, 1]]
    assert np.array_equal(vals[:, list(EXACT)], g["reg_vals"][:, list(EXACT)])
    np.testing.assert_allclose(vals, g["reg_vals"], rtol=1e-5, atol=1e-6)
    assert np.array_equal(weights.sum(1), g["reg_weights_sum"])


# ------------------------------------------------------------------------------------------------------------ margins on the inputs
def margins_assign(anchors, slot_cfg, matched, unmatched, class_cfg, gt, on_edge=0):
    """the generator's conditions on assignment inputs: every heading (anchors and owned rows) 1e-3 rad from the snap decision, no
    owned real row summing to zero, every anchor's best overlap 1e-5 from both thresholds except exactly `on_edge` anchors that sit ON
    one (bit-equal).  Both division forms must give the same result."""
    anchors, gt = np.asarray(anchors, F), np.asarray(gt, F)
    heads = [anchors[:, 6]]
    for b in range(gt.shape[0]):
        n = scene_rows(gt[b])
        heads.append(gt[b, :n, 6])
        real = np.abs(gt[b, :n, :7]).sum(1) > 0
        s = gt[b, :n, :7].astype(np.float64).sum(1)
        assert np.all(np.abs(s[real]) > 1e-3), "a real box whose values sum to zero"
    h = np.concatenate(heads).astype(np.float64)
    lp = np.abs(h - np.floor(h / np.pi + 0.5) * np.pi)
    assert np.all(np.abs(lp - np.pi / 4) > 1e-3), "a heading within 1e-3 rad of the snap decision"
    r = restate_assign(anchors, slot_cfg, matched, unmatched, class_cfg, gt, True, details=True)
    r2 = restate_assign(anchors, slot_cfg, matched, unmatched, class_cfg, gt, False, details=True)
    for x, y in zip(r, r2):
        assert np.array_equal(x, y), "the two division forms disagree"
    mine = np.asarray(slot_cfg)[np.arange(anchors.shape[0]) % len(slot_cfg)]
    has, best = r[3] >= 0, r[4]
    edge = 0
    for thr in (np.asarray(matched, F)[mine], np.asarray(unmatched, F)[mine]):
        d = np.abs(best.astype(np.float64) - thr[None].astype(np.float64))
        on = has & (best == thr[None])
        edge += int(on.sum())
        assert np.all(d[has & ~on] > 1e-5), "a best overlap within 1e-5 of a threshold"
    assert edge == on_edge, "%d anchors sit on a threshold, expected %d" % (edge, on_edge)
    return r


def margins_decode(box_preds, anchors, dir_cls_preds, off, lim, bins):
    t, a = np.asarray(box_preds, np.float64), np.asarray(anchors, np.float64)[None]
    if dir_cls_preds is None:
        return
    d = np.sort(np.asarray(dir_cls_preds, np.float64), axis=-1)
    assert bins < 2 or np.all(d[..., -1] - d[..., -2] > 1e-6), "tied direction logits"
    q = (t[..., 6] + a[..., 6] - off) / (2 * np.pi / bins) + lim
    assert np.all(np.abs(q - np.round(q)) > 1e-4), "val / period + offset within 1e-4 of an integer"


# ---------------------------------------------------------------------------------------------------------------------- seeded inputs
SIZES = {1: (3.9, 1.6, 1.56), 2: (0.8, 0.6, 1.73), 3: (1.76, 0.6, 1.73), 4: (5.0, 1.9, 2.1)}


def random_boxes(rng, n, num_class, rng_xy, pad=0):
    """(n + pad, 8) float32: n seeded boxes inside rng_xy = (x0, y0, x1, y1) with headings 0.05 rad clear of the snap decision, classes
    1..num_class, then `pad` zero rows"""
    out = np.zeros((n + pad, 8), F)
    for i in range(n):
        c = int(rng.integers(1, num_class + 1))
        size = np.array(SIZES.get(c, SIZES[1])) * rng.uniform(0.8, 1.25, 3)
        while True:
            r = rng.uniform(-np.pi, np.pi)
            if abs(abs(r - np.floor(r / np.pi + 0.5) * np.pi) - np.pi / 4) > 0.05:
                break
        out[i] = [rng.uniform(rng_xy[0], rng_xy[2]), rng.uniform(rng_xy[1], rng_xy[3]), rng.uniform(-1.5, -0.5), size[0], size[1], size[2], r, c]
    return out
