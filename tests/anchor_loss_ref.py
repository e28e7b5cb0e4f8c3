"""Float64 restatement of include/btcdet_hip_anchor_loss.h (btc_anchor_loss_fwd / _bwd) with a derived error bound for every output,
the seeded inputs of the shared case lists and the checks the anchor-loss test modules run.  Plain numpy: no GPU, no autograd.  The
conventions are those of tests/loss_ref.py: `ratio` above 1 is a failure, float arguments are float64(float32(v)), and the gradients
take the KERNEL's norms.

restate(d, dt, own, defect, norms_k, g) is ONE statement of the arithmetic, in the header's order of operations:
  dt = float64                the reference values (and the intermediates the bounds are built from)
  dt = float32                an emulation of the kernel: every numpy operation rounds to float32 on its own, sums in float64
  own = True                  the reference's OWN constants instead of the header's: beta = 1/9, 2 pi and dir_offset as doubles, true
                              divisions, weights as doubles -- what its float64 record was computed with
  defect                      one of DEFECTS: a seeded mistake, for showing that the checks can fail

Notation: u = 2^-24 (one correctly rounded fp32 operation, relative).  The library is built with -ffp-contract=off.  ASSUMED, as in
loss_ref.py: 2 ulp = 4 u = F for expf / logf / log1pf (relative), and the same 2 ulp for sinf / cosf on |x| <= 2 pi taken as an
ABSOLUTE F on each value (|sin|, |cos| <= 1).  A subnormal expf result may be flushed: FLOOR = 2^-125 absolute.  Every elementwise bound
is K = 2 times the first-order count below.

class term, x the logit, t the target bit, e = expf(-|x|):   A_e = F e + FLOOR
    r = 1 / (1 + e):  rel_r = A_e / (1 + e) + 2 u ;  p = r (x >= 0): A_p = p rel_r ;  p = e r: A_p = p (F + rel_r + u) + FLOOR
    om = 1 - p: A_om = A_p + u om        (ABSOLUTE 2^-24-sized errors on pt = om for a confident positive: the reference's own form)
    l = log1pf(e): A_l = A_e / (1 + e) + F l ;  bce = lin + l (lin exact): A_bce = A_l + u bce
    w = alpha (pt pt): A_w = alpha (2 pt A_pt + u pt^2) + u w ;  term = w bce: A_term = A_w bce + w A_bce + u term
    inner = (2 qt) bce + pt: A_inner = 2 A_qt bce + 2 qt A_bce + u (2 qt bce) + A_pt + u inner
    gc = w inner: A_gc = A_w inner + w A_inner + u gc ;  d_cls = s_0 gc, s_0 = (g norms_k) c_0: A = |s_0| A_gc + 4 u |d_cls|
location, column k: d = u_k - v_k.  k < 6: A_d = u |d|.  k = 6: u = sp ct, v = cp st with A_sin = A_cos = F:
    A_u = F (|ct| + |sp|) + u |u|, A_v likewise, A_d = A_u + A_v + u |d| ;  chain = cp ct + sp st: A_chain = F (|cp| + |ct| + |sp| + |st|) + 3 u
    n < beta: term = 0.5 n n / beta: A = (n / beta) A_d + 2 u term ;  else term = n - 0.5 beta: A = A_d + u term.  At n = beta both
    branches give beta / 2 and their slopes agree, so a comparison decided the other way by A_d costs A_d^2 / (2 beta): nothing.
    gr = d / beta or sign(d): A_gr = A_d / beta + u |gr| where n < beta + A_d, else 0 (exactly +-1)
    d_box = (s_1 gr) chain: A = |s_1| (A_gr |chain| + |gr| A_chain) + 5 u |d_box|
direction: dz_j = z_j - m <= 0, ez_j = expf(dz_j): A_ez = ez (u |dz| + F) + FLOOR ;  s = sum ez: A_s = sum A_ez + (bins - 1) u s
    term = logf(s) - (z_k - m): A = A_s / s + F |log s| + u |z_k - m| + u |term|
    soft_j = ez_j / s: A_soft = (A_ez + ez A_s / s) / s + u soft ;  d_dir = s_2 (soft - [j = k]): A = |s_2| (A_soft + u |soft - [j = k]|) + 4 u |d_dir|
    the bin k is an integer decision: the cases keep a margin of 1e-4 around an integer quotient (margins_dir), so either division form
    decides alike and the bound does not cover it
out[q] (double sums, one rounding to fp32): 2^-23 |ref| + 2^-40 sum |terms| + K sum A_term, each weighted weight_q / (B n_b)
out[3] = fp32(out[0] + fp32(out[1] + out[2])) of the kernel's own three values, norms[b] = fp32(1 / n_b): bit-exact.
Exact too: zeros at excluded gradients, and a d_box column k < 6 whose fp32 difference has n >= beta holds +-(g norms_k[b]) c_1 bit for
bit -- the check that sees a beta one ulp off (a one-ulp change of beta moves every VALUE by about u, below any bound).

tests/test_anchor_loss_cpu.py ties the restatement to the reference's float64 record at 1e-12, runs the float32 emulation over the case
lists below and shows for each of DEFECTS that some listed case fails."""
import json
import os
import zlib

import numpy as np

import anchor_targets_ref as ar
import loss_ref
from bn_ref import TINY, f32, ratio, wide
from loss_ref import F, FLOOR, K, U, sum_bound

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "anchor_loss.npz")
THREADS, MAX_TILES, MAX_BINS, MAX_CLASSES = 256, 512, 16, 64       # the header's constants
BETA32 = np.float32(1.0 / 9.0)
TWO_PI32 = np.float32(2.0 * np.pi)
CODE_W = np.array([1, 1, 1, 1, 1, 1, 0.2])                         # the `code_weights` defect applies these
DEFECTS = ("no_norm", "batch_norm", "beta_ulp", "dir_bin_shift", "ignored_as_background", "code_weights")
STAGES = ("out_cls", "out_loc", "out_dir", "out_total", "norms", "d_cls", "d_box", "d_dir", "seam")
EXACT = ("out_total", "norms", "seam")
W_DEFAULT = dict(cls_weight=1.0, loc_weight=2.0, dir_weight=0.2)
DIR_OFFSET = 0.78539
G_UP = 0.7


class Worst(loss_ref.Worst):
    """loss_ref.Worst over this module's stages"""

    def check(self, stage, got, ref_bound, where=""):
        assert stage in STAGES and stage not in EXACT, stage
        return self._note(stage, ratio(got, *ref_bound), where)

    def exact(self, stage, got, ref, where=""):
        assert stage in EXACT, stage
        got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
        same = got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got.view(np.uint8), ref.view(np.uint8))
        return self._note(stage, 0.0 if same else np.inf, where)

    def report(self):
        return "worst |got - ref| / bound: " + "  ".join(f"{s} {self.worst[s]:.3f}" for s in STAGES if s in self.worst)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def dir_bins(t6, a6, off, bins, T=np.float64, recip=True):
    """the header's direction bin (recip: multiplications by float32 reciprocals; else the reference's true divisions in doubles)"""
    with np.errstate(invalid="ignore"):
        v = (t6 + a6) - T(off)
        if recip:
            two_pi, inv, inv_w = T(TWO_PI32), T(np.float32(1.0) / TWO_PI32), T(np.float32(1.0) / np.float32(2.0 * np.pi / bins))
            lp = v - np.floor(v * inv) * two_pi
            kf = np.floor(lp * inv_w)
        else:
            lp = v - np.floor(v / (2 * np.pi)) * (2 * np.pi)
            kf = np.floor(lp / (2 * np.pi / bins))
    return np.clip(np.nan_to_num(kf, nan=0.0), 0, bins - 1).astype(np.int64)


def restate(d, dt=np.float64, own=False, defect=None, norms_k=None, g=1.0):
    """d: cls (B, A, C), box, tgt (B, A, 7), dir (B, A, bins) or None, labels (B, A), anchors (A, 7), w (dict), dir_offset
    -> dict: out (4), norms (B), d_cls, d_box, d_dir (None without bins), and the intermediates the bounds use"""
    assert defect is None or defect in DEFECTS
    T = dt
    cls, box, tgt = (np.asarray(d[k], np.float32).astype(T) for k in ("cls", "box", "tgt"))
    labels = np.asarray(d["labels"]).astype(np.int64)
    B, A, C = cls.shape
    dirs = None if d["dir"] is None else np.asarray(d["dir"], np.float32).astype(T)
    bins = 0 if dirs is None else dirs.shape[2]
    wq = [float(d["w"]["cls_weight"]), float(d["w"]["loc_weight"]), float(d["w"].get("dir_weight", 0.0)) if bins else 0.0]
    if not own:
        wq = [f32(v) for v in wq]
    beta = T(1.0 / 9.0) if own else T(BETA32)
    if defect == "beta_ulp":
        beta = T(np.nextafter(BETA32, np.float32(1)))
    pos, cared = labels > 0, labels >= 0
    if defect == "ignored_as_background":
        cared = np.ones_like(cared)
    nb = np.maximum(pos.sum(1), 1).astype(np.float64)
    if defect == "no_norm":
        nb = np.ones(B)
    elif defect == "batch_norm":
        nb = np.full(B, max(float(pos.sum()), 1.0))
    R = dict(B=B, A=A, C=C, bins=bins, pos=pos, cared=cared, nb=nb, wq=wq, beta=float(beta))
    with np.errstate(all="ignore"):
        # ---- class
        hot = np.where(pos, 1 if C == 1 else labels, 0)
        t = hot[..., None] == np.arange(1, C + 1)
        x = cls
        e = np.exp(-np.abs(x))
        r = T(1) / (T(1) + e)
        p = np.where(x >= 0, r, e * r)
        om = T(1) - p
        pt, qt = np.where(t, om, p), np.where(t, p, om)
        l = np.log1p(e)
        bce = (np.maximum(x, T(0)) - np.where(t, x, T(0))) + l
        w_ = np.where(t, T(0.25), T(0.75)) * (pt * pt)
        term_c = w_ * bce
        inner = (T(2) * qt) * bce + pt
        gc = w_ * inner
        cm = cared[..., None] & np.ones_like(t)
        R.update(x=x, t=t, e=e, p=p, om=om, pt=pt, qt=qt, l=l, bce=bce, w_=w_, inner=inner, gc=gc, cm=cm)
        term_c = np.where(cm, term_c, T(0))
        gc = np.where(cm, np.where(t, -gc, gc), T(0))
        # ---- location
        sp, cp, st, ct = np.sin(box[..., 6]), np.cos(box[..., 6]), np.sin(tgt[..., 6]), np.cos(tgt[..., 6])
        uu, vv = box.copy(), tgt.copy()
        uu[..., 6], vv[..., 6] = sp * ct, cp * st
        chain = np.ones_like(box)
        chain[..., 6] = cp * ct + sp * st
        live = ~np.isnan(vv) & pos[..., None]
        dd = np.where(live, uu - vv, T(0))
        if defect == "code_weights":
            dd = dd * CODE_W.astype(T)
        n = np.abs(dd)
        quad = n < beta
        sl = np.where(quad, T(0.5) * (n * n) / beta, n - T(0.5) * beta)
        gr = np.where(quad, dd / beta, np.sign(dd))
        if defect == "code_weights":
            gr = gr * CODE_W.astype(T)
        term_l = np.where(live, sl, T(0))
        R.update(sp=sp, cp=cp, st=st, ct=ct, uu=uu, vv=vv, chain=chain, live=live, dd=dd, n=n, quad=quad, sl=sl, gr=gr)
        # ---- direction
        term_d = np.zeros((B, A), T)
        if bins:
            a6 = np.asarray(d["anchors"], np.float32)[:, 6].astype(T)[None]
            k = dir_bins(tgt[..., 6], a6, d["dir_offset"] if own else np.float32(d["dir_offset"]), bins, T, recip=not own)
            if defect == "dir_bin_shift":
                k = (k + 1) % bins
            z = dirs
            m = z.max(-1)
            dz = z - m[..., None]
            ez = np.exp(dz)
            s = ez[..., 0].copy()
            for j in range(1, bins):
                s = s + ez[..., j]
            zk = np.take_along_axis(dz, k[..., None], -1)[..., 0]
            ce = np.log(s) - zk
            soft = ez / s[..., None]
            hit = k[..., None] == np.arange(bins)
            gd = soft - hit.astype(T)
            term_d = np.where(pos, ce, T(0))
            R.update(k=k, dz=dz, ez=ez, s=s, zk=zk, ce=ce, soft=soft, gd=gd)
    # ---- sums: float64 over the scene, then the header's double expression
    S = np.stack([wide(term_c).sum((1, 2)), wide(term_l).sum((1, 2)), wide(term_d).sum(1)])          # (3, B)
    Sabs = np.stack([np.abs(wide(term_c)).sum((1, 2)), np.abs(wide(term_l)).sum((1, 2)), np.abs(wide(term_d)).sum(1)])
    out = np.array([(S[q] / nb).sum() / B * wq[q] for q in range(3)])
    R["terms_abs"] = np.array([(Sabs[q] / nb).sum() / B * abs(wq[q]) for q in range(3)])
    norms = 1.0 / nb
    if T is np.float32:
        o = out.astype(np.float32)
        out = np.array([o[0], o[1], o[2], o[0] + (o[1] + o[2])], np.float32)
        norms = norms.astype(np.float32)
    else:
        out = np.array([out[0], out[1], out[2], out[0] + (out[1] + out[2])])
    R.update(out=out, norms=norms)
    # ---- gradients from the kernel's norms (its own when none are given)
    nk = (np.asarray(norms_k, np.float32) if norms_k is not None else np.asarray(norms)).astype(T)
    if own:
        sq = [T(g) * nk * T(wq[q] / B) for q in range(3)]
    else:
        gn = T(np.float32(g)) * nk
        sq = [gn * T(np.float32(wq[q]) / np.float32(B)) for q in range(3)]
    R["sq"] = [wide(v) for v in sq]
    with np.errstate(all="ignore"):
        R["d_cls"] = sq[0][:, None, None] * gc
        R["d_box"] = np.where(live, (sq[1][:, None, None] * gr) * chain, T(0))
        R["d_dir"] = np.where(pos[..., None], sq[2][:, None, None] * gd, T(0)) if bins else None
    return R


def bounds(R):
    """R = restate(d) in float64 with the header's constants -> dict of (ref, bound) per checked stage"""
    B, nb, wq = R["B"], R["nb"], R["wq"]
    out = {}
    with np.errstate(all="ignore"):
        # ---- class
        e, p, om, pt, qt, l, bce, w_, inner, t, x = (R[k] for k in ("e", "p", "om", "pt", "qt", "l", "bce", "w_", "inner", "t", "x"))
        a_e = F * e + FLOOR
        rel_r = a_e / (1 + e) + 2 * U
        a_p = np.where(x >= 0, p * rel_r, p * (F + rel_r + U) + FLOOR)
        a_om = a_p + U * om
        a_pt, a_qt = np.where(t, a_om, a_p), np.where(t, a_p, a_om)
        a_bce = a_e / (1 + e) + F * l + U * bce
        alpha = np.where(t, 0.25, 0.75)
        a_w = alpha * (2 * pt * a_pt + U * pt * pt) + U * w_
        a_term = np.where(R["cm"], a_w * bce + w_ * a_bce + U * w_ * bce, 0.0)
        a_inner = 2 * a_qt * bce + 2 * qt * a_bce + U * 2 * qt * bce + a_pt + U * inner
        a_gc = a_w * inner + w_ * a_inner + U * R["gc"]
        s0 = np.abs(R["sq"][0])[:, None, None]
        out["d_cls"] = (R["d_cls"], np.where(R["cm"], K * (s0 * a_gc + 4 * U * np.abs(R["d_cls"])), 0.0) + TINY)
        # ---- location
        sp, cp, st, ct, dd, n, quad, sl, gr, chain, live = (R[k] for k in ("sp", "cp", "st", "ct", "dd", "n", "quad", "sl", "gr", "chain", "live"))
        a_d = U * np.abs(dd)
        a_d[..., 6] = F * (np.abs(ct) + np.abs(sp)) + U * np.abs(R["uu"][..., 6]) + F * (np.abs(st) + np.abs(cp)) + U * np.abs(R["vv"][..., 6]) + U * np.abs(dd[..., 6])
        a_chain = np.zeros_like(dd)
        a_chain[..., 6] = F * (np.abs(cp) + np.abs(ct) + np.abs(sp) + np.abs(st)) + 3 * U
        a_sl = np.where(live, np.where(quad, n / R["beta"] * a_d + 2 * U * sl, a_d + U * sl), 0.0)
        a_gr = np.where(n < R["beta"] + a_d, a_d / R["beta"] + U * np.abs(gr), 0.0)
        s1 = np.abs(R["sq"][1])[:, None, None]
        out["d_box"] = (R["d_box"], np.where(live, K * (s1 * (a_gr * np.abs(chain) + np.abs(gr) * a_chain) + 5 * U * np.abs(R["d_box"])), 0.0) + TINY)
        # ---- direction
        a_ce = np.zeros(R["pos"].shape)
        if R["bins"]:
            dz, ez, s, zk, ce, soft, gd = (R[k] for k in ("dz", "ez", "s", "zk", "ce", "soft", "gd"))
            a_ez = ez * (U * np.abs(dz) + F) + FLOOR
            a_s = a_ez.sum(-1) + (R["bins"] - 1) * U * s
            a_ce = np.where(R["pos"], a_s / s + F * np.abs(np.log(s)) + U * np.abs(zk) + U * np.abs(ce), 0.0)
            a_soft = (a_ez + ez * (a_s / s)[..., None]) / s[..., None] + U * soft
            s2 = np.abs(R["sq"][2])[:, None, None]
            out["d_dir"] = (R["d_dir"], np.where(R["pos"][..., None], K * (s2 * (a_soft + U * np.abs(gd)) + 4 * U * np.abs(R["d_dir"])), 0.0) + TINY)
    per = [a_term.sum((1, 2)), a_sl.sum((1, 2)), a_ce.sum(1)]
    for q, name in enumerate(("out_cls", "out_loc", "out_dir")):
        per_term = K * (per[q] / nb).sum() / B * abs(wq[q])
        out[name] = (R["out"][q:q + 1], np.array([sum_bound(R["out"][q], R["terms_abs"][q], per_term)]))
    return out


def seam_expected(d, norms_k, g):
    """columns k < 6 of positive anchors whose float32 difference has n >= beta: (mask, the exact float32 d_box there)"""
    box, tgt = np.asarray(d["box"], np.float32), np.asarray(d["tgt"], np.float32)
    with np.errstate(all="ignore"):
        dd = box - tgt
        mask = (np.asarray(d["labels"]) > 0)[..., None] & ~np.isnan(tgt) & (np.abs(dd) >= BETA32)
        mask[..., 6] = False
        B = box.shape[0]
        s1 = (np.float32(g) * np.asarray(norms_k, np.float32)) * (np.float32(d["w"]["loc_weight"]) / np.float32(B))
        want = (s1[:, None, None] * np.sign(dd)).astype(np.float32)
    return mask, want


def check_anchor(W, d, got, where=""):
    """got: out (4), norms (B), d_cls, d_box, d_dir (None without bins), g (the upstream gradient the backward ran with) -- float32"""
    R = restate(d, norms_k=got["norms"], g=got["g"])
    bd = bounds(R)
    o = np.asarray(got["out"], np.float32)
    for q, name in enumerate(("out_cls", "out_loc", "out_dir")):
        W.check(name, o[q:q + 1], bd[name], where)
    W.exact("out_total", o[3], o[0] + (o[1] + o[2]), where)
    W.exact("norms", np.asarray(got["norms"], np.float32), (1.0 / R["nb"]).astype(np.float32), where)
    W.check("d_cls", got["d_cls"], bd["d_cls"], where)
    W.check("d_box", got["d_box"], bd["d_box"], where)
    if R["bins"]:
        W.check("d_dir", got["d_dir"], bd["d_dir"], where)
        W.require(not np.any(got["d_dir"][~R["pos"]]), f"{where}: d_dir at a non-positive anchor")
    else:
        W.require(got["d_dir"] is None and float(o[2]) == 0.0, where)
    labels = np.asarray(d["labels"])
    W.require(not np.any(got["d_cls"][labels < 0]), f"{where}: d_cls at an ignored anchor")
    W.require(not np.any(got["d_box"][labels <= 0]), f"{where}: d_box at a non-positive anchor")
    mask, want = seam_expected(d, got["norms"], got["g"])
    W.exact("seam", np.asarray(got["d_box"], np.float32)[mask], want[mask], where)
    W.require(np.isfinite(o).all() and np.isfinite(got["norms"]).all(), where)


def emulate(d, defect=None, g=G_UP):
    """the float32 emulation of both launches, in the shape check_anchor takes"""
    R = restate(d, dt=np.float32, defect=defect, g=g)
    return dict(out=R["out"], norms=R["norms"], d_cls=R["d_cls"], d_box=R["d_box"], d_dir=R["d_dir"], g=g)


# ------------------------------------------------------------------------------------------------------------------ margins
def margins_dir(d, margin=1e-4, on_clamp=None):
    """the generator's condition on direction inputs: at every positive anchor the bin quotient lies `margin` from an integer, and both
    division forms pick the same bin.  on_clamp (B, A) bool: anchors MEANT to sit just below a whole turn, where the quotient reaches
    `bins` in float32 and the clamp brings it back -- exempt from the margin, held to bin bins - 1 in both forms"""
    if d["dir"] is None:
        return
    pos = np.asarray(d["labels"]) > 0
    held = pos if on_clamp is None else pos & ~on_clamp
    t6, a6 = wide(d["tgt"])[..., 6], wide(d["anchors"])[None, :, 6]
    bins = d["dir"].shape[2]
    with np.errstate(all="ignore"):
        v = t6 + a6 - d["dir_offset"]
        q = (v - np.floor(v / (2 * np.pi)) * 2 * np.pi) / (2 * np.pi / bins)
        ok = ~held | np.isnan(q) | (np.abs(q - np.round(q)) > margin)
        # the quotient of limit_period itself: an integer there moves lp by a whole turn (bin bins -> the clamp), so it keeps the margin too
        q0 = v / (2 * np.pi)
        ok &= ~held | np.isnan(q0) | (np.abs(q0 - np.round(q0)) > margin / bins)
    assert np.all(ok), "a direction quotient within %g of an integer" % margin
    k1 = dir_bins(np.asarray(d["tgt"], np.float32)[..., 6], np.asarray(d["anchors"], np.float32)[None, :, 6], np.float32(d["dir_offset"]), bins, np.float32)
    k2 = dir_bins(t6, a6, d["dir_offset"], bins, np.float64, recip=False)
    assert np.array_equal(k1[pos], k2[pos]), "the two division forms disagree"
    if on_clamp is not None:
        assert on_clamp.any() and np.all(k1[pos & on_clamp] == bins - 1), "the clamp case does not sit on the upper clamp"


# ------------------------------------------------------------------------------------------------------------------ case lists
SHAPE_A = [0, 1, 63, 64, 65, 255, 256, 257, 513]
# one sweep of the capped grid covers MAX_TILES * THREADS anchors of a scene: one below, at, above, and a ragged second sweep
CAP = MAX_TILES * THREADS
CAP_A = [CAP - 1, CAP, CAP + 1, CAP + THREADS + 37]
VALUE_KINDS = ["logit_edges", "beta_seam", "heading_pi", "all_pos", "all_ign", "one_scene_pos", "nan_target"]
LOGIT_EDGES = [0.0, 20.0, -20.0, 90.0, -90.0, 1.5, -0.5]


def shape_cases():
    out = [dict(B=B, A=A, C=C, bins=bins, kind="random") for A in SHAPE_A for (B, C, bins) in ((1, 1, 0), (2, 3, 2), (3, 1, 2), (3, 3, 0))]
    return out


def cap_cases():
    return [dict(B=1, A=A, C=1, bins=2, kind="random") for A in CAP_A] + [dict(B=2, A=CAP + THREADS + 37, C=3, bins=0, kind="random")]


def value_cases():
    return [dict(B=3, A=257, C=C, bins=bins, kind=kind) for kind in VALUE_KINDS for (C, bins) in ((1, 2), (3, 0))]


KITTI_CASE = dict(B=2, A=70400, C=1, bins=2, kind="random")


def case_name(c):
    return "-".join(str(v) for v in c.values())


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def clear_dir_margins(d, margin=1e-3):
    """move the few headings whose bin quotient (or whole-turn quotient) lies near an integer"""
    if d["dir"] is None:
        return
    bins = d["dir"].shape[2]
    for _ in range(4):
        with np.errstate(all="ignore"):
            v = wide(d["tgt"])[..., 6] + wide(d["anchors"])[None, :, 6] - d["dir_offset"]
            q = v / (2 * np.pi / bins)
            near = np.abs(q - np.round(q)) < margin
        if not near.any():
            break
        d["tgt"][..., 6] += np.where(near, np.float32(0.01), np.float32(0))


def make_case(c, poison=True):
    """seeded inputs of one case; poison: what the labels exclude holds NaN, else zeros"""
    B, A, C, bins, kind = c["B"], c["A"], c["C"], c["bins"], c["kind"]
    rng = np.random.default_rng(_seed("anchor_loss", *c.values()))
    f = np.float32
    anchors = np.concatenate([rng.uniform(-20, 20, (A, 3)), rng.uniform(0.5, 4.0, (A, 3)), np.tile([0.0, 1.57], A)[:A, None]], axis=1).astype(f)
    u = rng.random((B, A))
    labels = np.where(u < 0.1, -1, np.where(u < 0.3, rng.integers(1, C + 1, (B, A)), 0)).astype(np.int32)
    if C == 1:                                  # class ids above 1 with one class: what a class-agnostic head is handed
        labels = np.where(labels > 0, rng.integers(1, 4, (B, A)), labels).astype(np.int32)
    cls = (rng.standard_normal((B, A, C)) * 2).astype(f)
    box = (rng.standard_normal((B, A, 7)) * 0.4).astype(f)
    tgt = (box + rng.standard_normal((B, A, 7)) * 0.15).astype(f)
    tgt[..., 6] = rng.uniform(-np.pi, np.pi, (B, A)).astype(f)
    box[..., 6] = (tgt[..., 6] + rng.standard_normal((B, A)) * 0.2).astype(f)
    dirs = rng.standard_normal((B, A, bins)).astype(f) if bins else None
    if kind == "logit_edges":
        k = (np.arange(B * A * C).reshape(B, A, C) + int(rng.integers(0, 7))) % len(LOGIT_EDGES)
        cls = np.array(LOGIT_EDGES, f)[k]
    elif kind == "beta_seam":                   # tgt = 0 in columns 0..5: d = box exactly; 0, +-beta, its float32 neighbours, +-1e3
        up, dn = np.nextafter(BETA32, f(1)), np.nextafter(BETA32, f(0))
        edges = np.array([0.0, BETA32, -BETA32, up, -up, dn, -dn, 1e3, -1e3], f)
        k = (np.arange(B * A * 6).reshape(B, A, 6) + int(rng.integers(0, 9))) % 9
        box[..., :6], tgt[..., :6] = edges[k], 0
        labels[:, ::2] = np.maximum(labels[:, ::2], 1)
    elif kind == "heading_pi":                  # the heading difference across +-pi, and a whole turn apart
        k = np.arange(B * A).reshape(B, A) % 4
        tgt[..., 6] = np.array([3.1, -3.1, 3.0, -2.5], f)[k]
        box[..., 6] = np.array([-3.1, 3.1, 3.0 - 2 * np.pi, -2.5 + np.pi], f)[k] + (rng.standard_normal((B, A)) * 0.01).astype(f)
        labels[:, ::2] = np.maximum(labels[:, ::2], 1)
    elif kind == "all_pos":
        labels = np.maximum(labels, 1).astype(np.int32)
    elif kind == "all_ign":
        labels[:] = -1
    elif kind == "one_scene_pos":
        labels[0], labels[B - 1] = np.minimum(labels[0], 0), np.minimum(labels[B - 1], 0)
    elif kind == "nan_target":
        hole = rng.random((B, A, 7)) < 0.2
        tgt[hole & (np.arange(7) != 6)] = np.nan                       # a NaN heading would also reach the direction bin
        labels[:, ::2] = np.maximum(labels[:, ::2], 1)
    d = dict(cls=cls, box=box, dir=dirs, labels=labels, tgt=tgt, anchors=anchors, w=dict(W_DEFAULT), dir_offset=DIR_OFFSET)
    clear_dir_margins(d)
    margins_dir(d)
    bad = f(np.nan) if poison else f(0)
    ign, nonpos = labels < 0, labels <= 0
    d["cls"][ign] = bad
    d["box"][nonpos], d["tgt"][nonpos] = bad, bad
    if bins:
        d["dir"][nonpos] = bad
    return d


# the two small heads of tests/golden/anchor_loss.npz: 8 x 8 locations x 2 rotations (A = 128), 5 x 7 locations x 3 configurations (A = 210)
GOLD_MAPS = {
    "car": dict(grid_size=[64, 64, 40], point_cloud_range=[0.0, -8.0, -3.0, 16.0, 8.0, 1.0], class_names=["Car"],
                generator=[ar._gen("Car", (3.9, 1.6, 1.56), -1.78, 0.6, 0.45)]),
    "three": dict(grid_size=[56, 40, 40], point_cloud_range=[0.0, -10.0, -3.0, 28.0, 10.0, 1.0], class_names=["Car", "Pedestrian", "Cyclist"],
                  generator=[ar._gen("Car", (3.9, 1.6, 1.56), -1.78, 0.6, 0.45), ar._gen("Pedestrian", (0.8, 0.6, 1.73), -0.6, 0.5, 0.35),
                             ar._gen("Cyclist", (1.76, 0.6, 1.73), -0.6, 0.5, 0.35)]),
}


def gold_cfg(map_name, with_dir=True, **loss_extra):
    """the DENSE_HEAD configuration of a golden map"""
    tgt = dict(NAME="AxisAlignedTargetAssigner", POS_FRACTION=-1.0, SAMPLE_SIZE=512, NORM_BY_NUM_EXAMPLES=False, MATCH_HEIGHT=False, BOX_CODER="ResidualCoder")
    cfg = dict(CLASS_AGNOSTIC=False, DIR_OFFSET=DIR_OFFSET, DIR_LIMIT_OFFSET=0.0, NUM_DIR_BINS=2, ANCHOR_GENERATOR_CONFIG=[dict(g) for g in GOLD_MAPS[map_name]["generator"]],
               TARGET_ASSIGNER_CONFIG=tgt, LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(W_DEFAULT, code_weights=[1.0] * 7), **loss_extra))
    if with_dir:
        cfg["USE_DIRECTION_CLASSIFIER"] = True
    return ar.ED(cfg)


def gold():
    g = np.load(GOLD)
    return g, json.loads(str(g["cases"]))


def gold_case(g, name, bins):
    """the recorded inputs of a golden case as a case dict"""
    return dict(cls=g[name + "/cls"], box=g[name + "/box"], dir=g[name + "/dir"] if bins else None, labels=g[name + "/labels"].astype(np.int32),
                tgt=g[name + "/tgt"], anchors=g[name + "/anchors"], w=dict(W_DEFAULT), dir_offset=DIR_OFFSET)
