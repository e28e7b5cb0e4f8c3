"""Numpy restatement of include/btcdet_hip_roi_targets.h (btc_roi_targets): the 3-D IoU from a BEV overlap, the masked max, the sampler, the
gather, the labels and the canonical transform, with the shared case lists, `margins`, a few seeded defects and the derived bound of the
two rotated columns.  Plain numpy: no GPU, no torch.

Every stage takes `dt`:
  dt = float32   an emulation of the kernel: every numpy operation rounds to float32 on its own (the library is built with
                 -ffp-contract=off); thresholds and constants are the float32 values the header names
  dt = float64   the reference values: the same constants (as float64(float32(v))), exact arithmetic to double precision
The BEV overlap itself (box_overlap of csrc/iou3d_dev.h) is NOT restated: a GPU test takes it from btc_boxes_pairwise_bev mode 0 on the same
boxes, a CPU test from `analytic_bev` -- the listed cases are built so that it is known in closed form (a roi is its box again, scaled
about its centre, turned by half a turn, pushed half a length along its own axis, or far from every box).

What is exact and what is bounded.  Every operation of the header but sinf / cosf is one correctly rounded float32 operation (fmodf is
exact), and the sampler's doubles (float32 uniform times an integer below 2^11: exact in double) are the same IEEE operations on either
side: max_overlaps, gt_assignment, sampled_inds, every gathered output, both label tensors, the heading column and lz are compared BIT FOR
BIT with the float32 emulation.  The two rotated columns are bounded with the conventions tests/anchor_loss_ref.py assumes: u = 2^-24,
sinf / cosf within 2 ulp = F = 4 u ABSOLUTE on each value for |x| <= 2 pi, K = 2 times the first-order count:
    ry = mod(r6): fmodf exact, the `+ two_pi` one rounding: A_ry = u |ry| ; c = cosf(-ry), s = sinf(-ry): A_c = A_s = F + A_ry
    lx = g0 - r0, ly = g1 - r1 (inputs exact): A_lx = u |lx|, A_ly = u |ly|
    x' = lx c - ly s: A = |lx| A_c + |ly| A_s + (A_lx |c| + A_ly |s|) + u (|lx c| + |ly s|) + u |x'|      (y' likewise with c, s swapped)
    bound = K A    (lx = ly = 0: both sides give exactly 0)
`margins` reports how far every threshold comparison (overlaps against the three candidate thresholds, sampled IoUs against the three label
thresholds) and every floor (u n of the draws, m HARD_BG_RATIO) is from flipping; `clear` holds the threshold margins to MARGIN.  The floors
cannot flip between the routes (same double operations); their distances are reported, and HARD_NUM_AT_INTEGER names the cases whose
m HARD_BG_RATIO is an integer in double (one of them, 70 x 0.7, only after rounding up from below)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import common  # noqa: E402

U = 2.0 ** -24
F_TRIG = 4 * U
K = 2
MARGIN = 1e-4
MAX_N = MAX_R = 1024
DEFECTS = ("tie_highest", "quota_without_no_background", "lists_swapped", "no_half_turn", "reg_valid_ge")


class Cfg(dict):
    __getattr__ = dict.__getitem__


def make_cfg(**kw):
    """the KITTI-Car TARGET_CONFIG with overrides"""
    return Cfg(dict(ROI_PER_IMAGE=128, FG_RATIO=0.5, SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou", CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25,
                    CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8, REG_FG_THRESH=0.55), **kw)


def consts(cfg, dt=np.float32):
    """the configuration block of the header: thresholds as float32 (held in dt), quota and span formed on the host"""
    f = lambda v: dt(np.float32(v))
    R = int(cfg.ROI_PER_IMAGE)
    return Cfg(R=R, fg_quota=int(round(float(cfg.FG_RATIO) * R)), reg_fg=f(cfg.REG_FG_THRESH), cls_fg=f(cfg.CLS_FG_THRESH), cls_bg=f(cfg.CLS_BG_THRESH),
               cls_bg_lo=f(cfg.CLS_BG_THRESH_LO), fg_thresh=f(min(cfg.REG_FG_THRESH, cfg.CLS_FG_THRESH)),
               cls_span=f(float(cfg.CLS_FG_THRESH) - float(cfg.CLS_BG_THRESH)), ratio=float(cfg.HARD_BG_RATIO))


# ---------------------------------------------------------------------------------------------------------------------- the stages
def iou3d(o, rois, gts, dt=np.float32):
    """o (N, G) BEV overlaps, rois (N, 7), gts (G, 8) -> (N, G) 3-D IoU"""
    a, b, o = rois.astype(dt), gts[:, :7].astype(dt), o.astype(dt)
    ha, hb = a[:, 5] / dt(2), b[:, 5] / dt(2)
    top = np.minimum((a[:, 2] + ha)[:, None], (b[:, 2] + hb)[None])
    bot = np.maximum((a[:, 2] - ha)[:, None], (b[:, 2] - hb)[None])
    h = np.maximum(top - bot, dt(0))
    o3 = o * h
    va, vb = (a[:, 3] * a[:, 4]) * a[:, 5], (b[:, 3] * b[:, 4]) * b[:, 5]
    den = np.maximum((va[:, None] + vb[None]) - o3, dt(np.float32(1e-6)))
    return o3 / den


def match(iou, labels, gts, by_class, defect=None):
    """-> (max_overlaps (N,), gt_assignment (N,) int64): the largest value, among equals the lowest box index"""
    val = iou
    if by_class:
        same = labels.astype(np.int64)[:, None] == gts[:, 7].astype(np.int64)[None]
        val = np.where(same, iou, iou.dtype.type(-1))
    if defect == "tie_highest":
        arg = val.shape[1] - 1 - np.argmax(val[:, ::-1], axis=1)
    else:
        arg = np.argmax(val, axis=1)
    best = val[np.arange(val.shape[0]), arg]
    if by_class:
        none = best < 0
        best, arg = np.where(none, best.dtype.type(0), best), np.where(none, 0, arg)
    return best, arg.astype(np.int64)


def _draw(u_row, n, R):
    return np.minimum(np.floor(u_row[:R].astype(np.float64) * float(n)).astype(np.int64), max(n, 1) - 1)


def quotas(n_fg, n_hard, n_easy, c, defect=None):
    R = c.R
    if n_easy + n_hard > 0 or defect == "quota_without_no_background":
        fg_this = min(n_fg, c.fg_quota)
    else:
        fg_this = R if n_fg > 0 else 0
    m = R - fg_this
    if n_hard > 0 and n_easy > 0:
        hard_num = min(int(np.floor(float(m) * c.ratio)), n_hard)
    else:
        hard_num = m if n_hard > 0 else 0
    return fg_this, m, hard_num


def sample(ov, u, cfg, defect=None):
    """ov (N,) float32 max_overlaps, u (4, max(R, N)) float32 -> sampled_inds (R,) int64"""
    c = consts(cfg)
    ov = ov.astype(np.float32)
    N, R = ov.shape[0], c.R
    fg, easy = ov >= c.fg_thresh, ov < c.cls_bg_lo
    hard = (ov < c.reg_fg) & (ov >= c.cls_bg_lo)
    n_fg, n_easy, n_hard = int(fg.sum()), int(easy.sum()), int(hard.sum())
    members = np.nonzero(fg)[0]
    fg_order = np.concatenate([members[np.lexsort((members, u[0, :N][members]))], np.nonzero(~fg)[0]])
    lists = [np.concatenate([np.nonzero(s)[0], np.nonzero(~s)[0]]) for s in (hard, easy)]
    hard_list, easy_list = lists[::-1] if defect == "lists_swapped" else lists
    fg_this, m, hard_num = quotas(n_fg, n_hard, n_easy, c, defect)
    j = np.arange(R)
    if n_easy + n_hard > 0:
        fg_idx = fg_order[np.minimum(j, N - 1)]
    else:
        fg_idx = fg_order[_draw(u[1], n_fg, R)]
    bg_idx = np.where(j - fg_this < hard_num, hard_list[_draw(u[2], n_hard, R)], easy_list[_draw(u[3], n_easy, R)])
    return np.where(j < fg_this, fg_idx, bg_idx).astype(np.int64)


def labels_of(iou, cfg, dt=np.float32, defect=None):
    """iou (..,) -> (reg_valid_mask int64, rcnn_cls_labels: dt for roi_iou, int64 for cls)"""
    c = consts(cfg, dt)
    iou = iou.astype(dt)
    reg = (iou >= c.reg_fg) if defect == "reg_valid_ge" else (iou > c.reg_fg)
    if cfg.CLS_SCORE_TYPE == "cls":
        cls = (iou > c.cls_fg).astype(np.int64)
        cls[(iou > c.cls_bg) & (iou < c.cls_fg)] = -1
    else:
        mid = (iou - c.cls_bg) * (dt(1) / c.cls_span) if dt is np.float32 else (iou - c.cls_bg) / c.cls_span
        cls = np.where(iou > c.cls_fg, dt(1), np.where(iou < c.cls_bg, dt(0), mid)).astype(dt)
    return reg.astype(np.int64), cls


def _angles(dt):
    f = lambda v: dt(np.float32(v))
    return f(2 * np.pi), f(np.pi), f(np.pi * 0.5), f(np.pi * 1.5)


def _mod(x, two_pi):
    m = np.fmod(x, two_pi)
    return np.where((m != 0) & (m < 0), m + two_pi, m)


def canonical(rois, gt, dt=np.float32, defect=None, parts=False):
    """rois (.., 7), gt (.., 8) -> gt_of_rois (.., 8) in the roi's frame (parts: also ry, lx, ly, c, s, x', y' for the bound)"""
    two_pi, pi, half_pi, three_half_pi = _angles(dt)
    r, g = rois.astype(dt), gt.astype(dt)
    ry = _mod(r[..., 6], two_pi)
    lx, ly, lz = g[..., 0] - r[..., 0], g[..., 1] - r[..., 1], g[..., 2] - r[..., 2]
    lh = g[..., 6] - ry
    c, s = np.cos(-ry), np.sin(-ry)
    x = lx * c - ly * s
    y = lx * s + ly * c
    hd = _mod(lh, two_pi)
    if defect != "no_half_turn":
        hd = np.where((hd > half_pi) & (hd < three_half_pi), _mod(hd + pi, two_pi), hd)
    hd = np.where(hd > pi, hd - two_pi, hd)
    hd = np.clip(hd, -half_pi, half_pi)
    out = np.stack([x, y, lz, g[..., 3], g[..., 4], g[..., 5], hd, g[..., 7]], axis=-1).astype(dt)
    return (out, dict(ry=ry, lx=lx, ly=ly, c=c, s=s, x=x, y=y)) if parts else out


def rotated_bound(rois, gt):
    """(.., 2): the bound of |kernel - float64 restatement| on columns 0 and 1 of gt_of_rois (the docstring's derivation)"""
    _, p = canonical(rois, gt, np.float64, parts=True)
    alx, aly, ac, as_ = np.abs(p["lx"]), np.abs(p["ly"]), np.abs(p["c"]), np.abs(p["s"])
    a_trig = F_TRIG + U * np.abs(p["ry"])
    first = (alx + aly) * a_trig
    bx = first + U * (alx * ac + aly * as_) + U * (alx * ac + aly * as_) + U * np.abs(p["x"])
    by = first + U * (alx * as_ + aly * ac) + U * (alx * as_ + aly * ac) + U * np.abs(p["y"])
    return K * np.stack([bx, by], axis=-1)


def restate(case, bev, dt=np.float32, defect=None, sampled_in=None):
    """the whole call on one case: bev (B, N, G) BEV overlaps -> the output dict of the header (numpy)"""
    cfg = case["cfg"]
    B, N = case["rois"].shape[:2]
    R = int(cfg.ROI_PER_IMAGE)
    out = {k: [] for k in ("max_overlaps", "gt_assignment", "sampled_inds", "rois", "gt_of_rois_src", "gt_iou_of_rois", "roi_scores", "roi_labels")}
    for b in range(B):
        iou = iou3d(bev[b], case["rois"][b], case["gt_boxes"][b], dt)
        ov, arg = match(iou, case["roi_labels"][b], case["gt_boxes"][b], bool(cfg.SAMPLE_ROI_BY_EACH_CLASS), defect)
        # the sampler sees the float32 overlaps on either setting of dt: it is the kernel's decision that is restated
        sel = sample(ov.astype(np.float32), case["uniforms"][b], cfg, defect) if sampled_in is None else np.clip(sampled_in[b], 0, N - 1)
        for k, v in (("max_overlaps", ov), ("gt_assignment", arg), ("sampled_inds", sel), ("rois", case["rois"][b][sel]),
                     ("gt_of_rois_src", case["gt_boxes"][b][arg[sel]]), ("gt_iou_of_rois", ov[sel]), ("roi_scores", case["roi_scores"][b][sel]),
                     ("roi_labels", case["roi_labels"][b][sel])):
            out[k].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    out["reg_valid_mask"], out["rcnn_cls_labels"] = labels_of(out["gt_iou_of_rois"], cfg, dt, defect)
    out["gt_of_rois"] = canonical(out["rois"], out["gt_of_rois_src"], dt, defect)
    assert out["sampled_inds"].shape == (B, R)
    return out


EXACT_KEYS = ("max_overlaps", "gt_assignment", "sampled_inds", "rois", "gt_of_rois_src", "gt_iou_of_rois", "roi_scores", "roi_labels", "reg_valid_mask",
              "rcnn_cls_labels")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_outputs(got, emu, ref64, what, keys=EXACT_KEYS + ("gt_of_rois",)):
    """got: a route's outputs; emu: restate(float32); ref64: restate(float64).  Exact keys bit for bit against the emulation, columns 2..7 of
    gt_of_rois too, columns 0 and 1 inside rotated_bound of the float64 values.  -> the worst ratio of the rotated columns"""
    for k in keys:
        if k == "gt_of_rois":
            continue
        assert same_bits(got[k], emu[k]), "%s: %s differs from the float32 restatement at %s" % (what, k, np.argwhere(np.asarray(got[k]) != emu[k])[:4].tolist())
    worst = 0.0
    if "gt_of_rois" in keys:
        g = got["gt_of_rois"]
        assert same_bits(g[..., 2:], emu["gt_of_rois"][..., 2:]), "%s: gt_of_rois columns 2..7 differ from the float32 restatement" % what
        bound = rotated_bound(got["rois"], got["gt_of_rois_src"])
        err = np.abs(g[..., :2].astype(np.float64) - ref64["gt_of_rois"][..., :2])
        ok = err <= bound
        assert ok.all(), "%s: rotated columns outside the bound: err %r bound %r" % (what, err[~ok][:4], bound[~ok][:4])
        worst = float(np.max(err / np.maximum(bound, 1e-300), initial=0.0))
    return worst


def margins(ov, iou_sel, uniforms, cfg):
    """ov (B, N) max_overlaps, iou_sel (B, R) sampled IoUs, uniforms (B, 4, M) -> the least distance of every comparison / floor from flipping"""
    c = consts(cfg, np.float64)
    R = c.R
    ov, iou_sel = np.asarray(ov, np.float64), np.asarray(iou_sel, np.float64)
    m = dict(candidates=min(float(np.abs(ov - t).min()) for t in (c.fg_thresh, c.cls_bg_lo, c.reg_fg)),
             labels=min(float(np.abs(iou_sel - t).min()) for t in (c.reg_fg, c.cls_fg, c.cls_bg)), draws=1.0, hard_num=1.0)
    for b in range(ov.shape[0]):
        o32 = ov[b].astype(np.float32)
        n_fg, n_easy = int((o32 >= np.float32(c.fg_thresh)).sum()), int((o32 < np.float32(c.cls_bg_lo)).sum())
        n_hard = int(((o32 < np.float32(c.reg_fg)) & (o32 >= np.float32(c.cls_bg_lo))).sum())
        fg_this, mm, _ = quotas(n_fg, n_hard, n_easy, c)
        for row, n in ((1, n_fg), (2, n_hard), (3, n_easy)):
            if n > 0:
                p = uniforms[b, row, :R].astype(np.float64) * n
                inner = p[p >= 1.0]     # (below 1 the floor is 0 and only a negative product could flip it)
                if inner.size:
                    m["draws"] = min(m["draws"], float((inner - np.floor(inner)).min()))
        if n_hard > 0 and n_easy > 0:
            q = float(mm) * c.ratio
            m["hard_num"] = min(m["hard_num"], q - np.floor(q), np.ceil(q) - q if np.ceil(q) > q else 1.0)
    return m


def clear(m):
    return m["candidates"] > MARGIN and m["labels"] > MARGIN


def foreground_keys_distinct(ov, uniforms, cfg):
    c = consts(cfg)
    for b in range(ov.shape[0]):
        keys = uniforms[b, 0, :ov.shape[1]][ov[b].astype(np.float32) >= c.fg_thresh]
        if np.unique(keys).size != keys.size:
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------------- the cases
# kinds of a roi around box g: F its box scaled about the centre by up to 2 % per axis (IoU above 0.88), every second one turned by half a
# turn; H its box pushed half a length along its own axis (IoU 1/3), every second one turned likewise; E far from every box (IoU 0)
def _spec(name, B, N, G, mix, **kw):
    return dict(dict(name=name, B=B, N=N, G=G, mix=mix, R=128, by_class=True, score="roi_iou", ratio=0.8, zero_scene=None, alien_scene=None, tie=False,
                     classes=1), **kw)


# mix = (foreground, hard) of scene 0, the rest easy; scene b > 0 of a case rotates the three counts
CASES = [
    _spec("n1_fg_only", 1, 1, 1, (1, 0)),                                               # foreground only: every slot drawn with replacement
    _spec("n63", 3, 63, 2, (20, 20), classes=2),
    _spec("n64_fg_only", 1, 64, 37, (64, 0), by_class=False),
    _spec("n65_no_fg", 1, 65, 1, (0, 30)),
    _spec("n127_quota_minus_1", 1, 127, 2, (63, 30)),                                   # m = 65: m * 0.8 = 52 exactly
    _spec("n128_quota", 3, 128, 37, (64, 30), classes=2, score="cls"),                  # m = 64: 51.2
    _spec("n257_quota_plus_1", 1, 257, 37, (65, 100), by_class=False),
    _spec("n129_m66", 1, 129, 2, (62, 40)),                                             # m = 66: 52.8
    _spec("n512_cls", 3, 512, 37, (170, 170), by_class=False, score="cls"),
    _spec("n1024", 1, 1024, 37, (300, 300), classes=2),
    _spec("n1024_r1024", 1, 1024, 2, (200, 100), R=1024),
    _spec("easy_only", 1, 100, 2, (0, 0)),
    _spec("hard_only", 1, 100, 2, (0, 100), score="cls"),
    _spec("zero_scene", 3, 65, 2, (30, 20), zero_scene=1),
    _spec("alien_class", 2, 127, 37, (50, 40), alien_scene=1, classes=2),
    _spec("alien_class_any", 2, 127, 37, (50, 40), alien_scene=1, classes=2, by_class=False),
    _spec("tie", 1, 65, 2, (30, 20), tie=True),
    _spec("tie_any_class", 1, 65, 2, (30, 20), tie=True, by_class=False),
    _spec("ratio_07_m70", 1, 200, 2, (58, 60), ratio=0.7),                              # 70 * 0.7 rounds to 49 in double, from below
    _spec("r32", 1, 512, 37, (100, 100), R=32),
    _spec("r200_n63", 1, 63, 2, (20, 20), R=200),
]
CASE_IDS = [c["name"] for c in CASES]
HARD_NUM_AT_INTEGER = ("n127_quota_minus_1", "ratio_07_m70", "r200_n63")


def make_case(spec):
    """-> dict(rois (B, N, 7), roi_scores (B, N), roi_labels (B, N) int64, gt_boxes (B, G, 8), uniforms (B, 4, M), cfg, kinds (B, N), base (B, N))"""
    B, N, G, R = spec["B"], spec["N"], spec["G"], spec["R"]
    salt = 7000 + 97 * CASE_IDS.index(spec["name"])
    h = lambda n, s: common._hash01(n, salt + s).astype(np.float64)
    cfg = make_cfg(ROI_PER_IMAGE=R, SAMPLE_ROI_BY_EACH_CLASS=spec["by_class"], CLS_SCORE_TYPE=spec["score"], HARD_BG_RATIO=spec["ratio"])
    n_real = G if G < 3 else G - G // 5                                 # wider lists end in zero-padded rows
    gts = np.zeros((B, G, 8), np.float32)
    rois = np.zeros((B, N, 7), np.float32)
    labels = np.ones((B, N), np.int64)
    kinds = np.zeros((B, N), np.int8)                                   # 0 easy, 1 hard, 2 foreground
    base = np.zeros((B, N), np.int64)
    for b in range(B):
        g = np.arange(n_real)
        u = h(n_real * 4, 10 + b).reshape(n_real, 4)
        box = np.zeros((n_real, 8))
        box[:, 0], box[:, 1], box[:, 2] = 10 + 12 * (g % 6), -36 + 12 * (g // 6), -1 + 0.4 * (u[:, 0] - 0.5)
        box[:, 3:6] = np.array([3.9, 1.6, 1.56]) * (1 + 0.2 * (u[:, 1:2] - 0.5))
        box[:, 6] = (u[:, 2] - 0.5) * 6.2
        box[:, 7] = 1 + (g % spec["classes"])
        if spec["tie"]:
            box[1] = box[0]
        if spec["zero_scene"] == b:
            box[:] = 0
        gts[b, :n_real] = box.astype(np.float32)
        box = gts[b, :n_real].astype(np.float64)                         # the rois are built from the float32 boxes
        nf, nh = spec["mix"]
        counts = [(nf, nh, N - nf - nh), (nh, N - nf - nh, nf), (0, nh, N - nh)][b % 3]
        counts = (counts[0], counts[1], N - counts[0] - counts[1])
        kind = np.concatenate([np.full(counts[0], 2), np.full(counts[1], 1), np.full(counts[2], 0)])[np.argsort(h(N, 20 + b), kind="stable")]
        k = np.arange(N)
        bi = k % n_real
        if spec["tie"]:
            bi = np.zeros(N, np.int64)
        v = h(N * 6, 30 + b).reshape(N, 6)
        r = box[bi, :7].copy()
        fgm, hdm, esm = kind == 2, kind == 1, kind == 0
        r[fgm, 3:6] *= 1 + 0.04 * (v[fgm, 0:3] - 0.5)
        r[hdm, 0] += 0.5 * r[hdm, 3] * np.cos(r[hdm, 6])
        r[hdm, 1] += 0.5 * r[hdm, 3] * np.sin(r[hdm, 6])
        turn = (k % 2 == 1) & ~esm
        r[turn, 6] += np.pi
        r[esm, 0], r[esm, 1] = 300 + 7 * k[esm], (v[esm, 3] - 0.5) * 40
        r[esm, 6] = (v[esm, 4] - 0.5) * 14                               # beyond +-2 pi: both branches of the floored mod
        if spec["zero_scene"] == b:                                      # no box: the rois stand where the boxes would have stood
            r[:, 0], r[:, 1], r[:, 2], r[:, 3:6] = 10 + 3 * k, (v[:, 3] - 0.5) * 40, -1, np.array([3.9, 1.6, 1.56])
            kind[:] = 0
        rois[b], kinds[b], base[b] = r.astype(np.float32), kind, bi
        labels[b] = gts[b, bi, 7].astype(np.int64) if spec["zero_scene"] != b else 1
        if spec["alien_scene"] == b:
            labels[b] = 3
    M = max(R, N)
    return dict(rois=rois, roi_scores=common._hash01(B * N, salt + 1).reshape(B, N), roi_labels=labels, gt_boxes=gts,
                uniforms=common._hash01(B * 4 * M, salt + 2).reshape(B, 4, M), cfg=cfg, kinds=kinds, base=base, spec=spec, batch_size=B)


def analytic_bev(case):
    """(B, N, G) float32: the BEV overlap of every (roi, box) pair of a listed case in closed form: a foreground roi and its box are
    concentric rectangles of one orientation (half a turn maps a rectangle onto itself), a hard roi covers half its box, nothing else
    touches (boxes 12 m apart, easy rois far away); a duplicated box (tie) overlaps like its twin"""
    rois, gts, kinds, base = case["rois"].astype(np.float64), case["gt_boxes"].astype(np.float64), case["kinds"], case["base"]
    B, N = rois.shape[:2]
    G = gts.shape[1]
    o = np.zeros((B, N, G))
    for b in range(B):
        for n in range(N):
            g = base[b, n]
            twins = [g] + ([1 - g] if case["spec"]["tie"] else [])
            for t in twins:
                if kinds[b, n] == 2:
                    o[b, n, t] = min(rois[b, n, 3], gts[b, t, 3]) * min(rois[b, n, 4], gts[b, t, 4])
                elif kinds[b, n] == 1:
                    o[b, n, t] = 0.5 * gts[b, t, 3] * gts[b, t, 4]
    return o.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the sampler-only cases
SAMPLER_CFG = Cfg(ROI_PER_IMAGE=128, FG_RATIO=0.5, REG_FG_THRESH=0.55, CLS_FG_THRESH=0.75, CLS_BG_THRESH=0.25, CLS_BG_THRESH_LO=0.1, HARD_BG_RATIO=0.8,
                  SAMPLE_ROI_BY_EACH_CLASS=True, CLS_SCORE_TYPE="roi_iou")


def sampler_overlaps(seed, n=None):
    """the overlap vectors of tests/test_roi_sampler_cpu.py (twelve seeds, six kinds); n overrides the drawn length"""
    rng = np.random.default_rng(seed)
    drawn = int(rng.integers(1, 600))
    n = drawn if n is None else n
    kind = seed % 6
    ov = rng.uniform(0, 1, n)
    if kind == 1:
        ov = rng.uniform(0.6, 1, n)
    elif kind == 2:
        ov = rng.uniform(0, 0.09, n)
    elif kind == 3:
        ov = rng.uniform(0.1, 0.5, n)
    elif kind == 4:
        ov = np.where(rng.uniform(0, 1, n) < 0.02, 0.9, rng.uniform(0, 0.5, n))
    elif kind == 5:
        ov = np.where(rng.uniform(0, 1, n) < 0.9, 0.9, 0.3)
    return ov.astype(np.float32)
