"""Restatement of include/btcdet_hip_roi_loss.h (btc_roi_loss_fwd / _bwd) with a derived error bound for every output, the seeded inputs
of the shared case lists and the checks the ROI-loss test modules run.  Plain numpy: no GPU, no autograd.  The conventions are those of
tests/loss_ref.py and tests/anchor_loss_ref.py: `ratio` above 1 is a failure, float arguments are float64(float32(v)), and the gradients
take the KERNEL's norms.

restate(d, dt, own, defect, norms_k, g) is ONE statement of the arithmetic, in the header's order of operations:
  dt = float64                the reference values
  dt = float32                an emulation of the kernel: every numpy operation rounds to float32 on its own, sums in float64
  dt = "err"                  float64 values that carry a bound on their error (class E below): the derivation of the bound, carried
                              along the very operations that are being bounded -- bounds() is this mode
  own = True                  the reference's OWN constants instead of the header's: beta = 1/9, pi, 1e-5 and 1e-12 as doubles, weights
                              as doubles -- what its float64 record was computed with
  defect                      one of DEFECTS: a seeded mistake, for showing that the checks can fail

How the bound is derived.  u = 2^-24 (one correctly rounded fp32 operation, relative); the library is built with -ffp-contract=off.
ASSUMED, as in loss_ref.py: 2 ulp = 4 u = F for expf / logf / sqrtf (relative), and the same 2 ulp for sinf / cosf on |x| <= 2 pi taken
as an ABSOLUTE F on each value (|sin|, |cos| <= 1) -- the bound-checked cases keep every trig argument inside that range (asserted by
make_case).  A subnormal expf result may be flushed: FLOOR = 2^-125 absolute.  An E value (v, a) says |computed - v| <= a, and
    z = x + y, x - y :  a_z = a_x + a_y + u |z|                    z = x y :  a_z = |x| a_y + |y| a_x + a_x a_y + u |z|
    z = x / y        :  a_z = a_x / |y| + |z| a_y / |y| + u |z|    exp: a_z = z a_x + F z + FLOOR      log: a_z = a_x / |x| + F |z|
    sqrt             :  a_z = min(a_x / z, sqrt(a_x)) + F z        (sqrt(x + e) - sqrt(x) = e / (sqrt(x + e) + sqrt(x)): holds at x = 0 too)
    sin, cos         :  a_z = a_x + F                              max(x, c), min with a constant, where: the error of what is taken
Inputs are exact.  A multiplication by 0.5 or 0.125 is charged like any other (the bound is then a little wider than needed, never
narrower).  Every elementwise bound is K = 2 times that count.  Where a comparison picks a branch, the branches are continuous:
    smooth L1 at n = beta and the corner term at m = 1: value and slope agree, a comparison decided the other way costs second order;
    gr = d / beta against sign(d): charged a_d / beta wherever n < beta + a_d, else exactly +-1;
    G = D against D / m: charged |D| a_m / m more wherever |m - 1| <= a_m.
The choice of the twin is NOT continuous in the gradient: the cases keep a margin around ties of the two distances (margins(),
asserted by make_case), so both implementations pick the same twin and the bound does not cover it.
The class term where p = sigmoid(x) rounds to 1.0f (x above 24 ln 2) is 100 (1 - t) by contract and its gradient exactly 0; where p
underflows (x <= -101 here) the term is 100 t and |gradient| <= 1e12 p < 2e-32, below the 1e-30 every bound carries.  The float64
value of these entries is NOT what the kernel owes, so the restatement takes the contract there in every mode; the cases keep valid
logits out of (10, 17) and (-101, -20) (asserted), where a float32 `1 - p` has few or no correct digits.
out[q] (double sums, one rounding to fp32): 2^-23 |ref| + 2^-40 sum |terms| + K sum a_term, each scaled by weight_q / n.
out[3] = fp32(out[1] + out[2]) and out[4] = fp32(out[0] + out[3]) of the kernel's own values, norms = fp32(1 / n): bit-exact.
Exact too: zeros at excluded gradients and at saturated logits; and, without the corner term, a d_reg column 2 or 6 (whose target is
a correctly rounded division or a copy) whose fp32 difference has n >= beta holds +-(g norms_k[1]) reg_weight bit for bit.

tests/test_roi_loss_cpu.py ties the restatement to the reference's float64 record at 1e-12, runs the float32 emulation over the case
lists below and shows for each of DEFECTS that some listed case fails."""
import json
import os
import re
import zlib

import numpy as np

import loss_ref
from bn_ref import TINY, f32, ratio, wide
from loss_ref import F, FLOOR, K, U, sum_bound

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "roi_loss.npz")
_HDR = open(os.path.join(os.path.dirname(HERE), "include", "btcdet_hip_roi_loss.h")).read()
THREADS = int(re.search(r"#define BTC_ROI_LOSS_THREADS (\d+)", _HDR).group(1))
LANES = int(re.search(r"#define BTC_ROI_LOSS_LANES (\d+)", _HDR).group(1))
MAX_TILES = int(re.search(r"#define BTC_ROI_LOSS_MAX_TILES (\d+)", _HDR).group(1))
TILE = THREADS // LANES
BETA32 = np.float32(1.0 / 9.0)
PI32 = np.float32(np.pi)
DEFECTS = ("no_twin", "corner_beta_ninth", "reg_by_valid", "per_scene_norm", "heading_not_zeroed", "clamped_decode", "ignored_as_background")
STAGES = ("out_cls", "out_reg", "out_corner", "out_regsum", "out_total", "norms", "d_cls", "d_reg", "seam", "sat")
EXACT = ("out_regsum", "out_total", "norms", "seam", "sat")
W_DEFAULT = dict(rcnn_cls_weight=1.0, rcnn_reg_weight=1.5, rcnn_corner_weight=0.75)
G_UP = 0.7
KIND_ROI_IOU, KIND_CLS = 0, 1
SAT_HI = 24.0 * np.log(2.0)        # 1 + expf(-x) rounds to 1 above this
HX = np.array([1, 1, -1, -1, 1, 1, -1, -1]) * 0.5
HY = np.array([1, -1, -1, 1, 1, -1, -1, 1]) * 0.5
HZ = np.array([-1, -1, -1, -1, 1, 1, 1, 1]) * 0.5


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


# ------------------------------------------------------------------------------------------------------------------ values with a bound
class E(object):
    """float64 values v with a bound a on |computed - v| (the module docstring's rules)"""
    __array_ufunc__ = None

    def __init__(self, v, a=0.0):
        self.v = np.asarray(v, np.float64)
        self.a = np.broadcast_to(np.asarray(a, np.float64), self.v.shape)

    @staticmethod
    def lift(o):
        return o if isinstance(o, E) else E(o)

    @staticmethod
    def _r(v, a):
        return E(v, a + U * np.abs(v))

    def __add__(self, o):
        o = E.lift(o)
        return E._r(self.v + o.v, self.a + o.a)

    __radd__ = __add__

    def __sub__(self, o):
        o = E.lift(o)
        return E._r(self.v - o.v, self.a + o.a)

    def __rsub__(self, o):
        return E.lift(o) - self

    def __mul__(self, o):
        o = E.lift(o)
        return E._r(self.v * o.v, np.abs(self.v) * o.a + np.abs(o.v) * self.a + self.a * o.a)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.lift(o)
        z = self.v / o.v
        return E._r(z, self.a / np.abs(o.v) + np.abs(z) * o.a / np.abs(o.v))

    def __rtruediv__(self, o):
        return E.lift(o) / self

    def __neg__(self):
        return E(-self.v, self.a)

    def __getitem__(self, i):
        return E(self.v[i], self.a[i])


def raw(x):
    return x.v if isinstance(x, E) else x


class Ops(object):
    """the library functions and selections of the restatement, for plain arrays (float32 / float64) and for E values"""

    def __init__(self, dt):
        self.err = isinstance(dt, str)
        assert not self.err or dt == "err"
        self.T = np.float64 if self.err else dt

    def inp(self, a):
        a = np.asarray(a, np.float32).astype(self.T)
        return E(a) if self.err else a

    def exp(self, x):
        if self.err:
            z = np.exp(x.v)
            return E(z, z * x.a + F * z + FLOOR)
        return np.exp(x)

    def log(self, x):
        if self.err:
            z = np.log(x.v)
            return E(z, x.a / np.abs(x.v) + F * np.abs(z))
        return np.log(x)

    def sqrt(self, x):
        if self.err:
            z = np.sqrt(x.v)
            return E(z, np.minimum(x.a / np.maximum(z, 1e-300), np.sqrt(x.a)) + F * z)
        return np.sqrt(x)

    def sin(self, x):
        return E(np.sin(x.v), x.a + F) if self.err else np.sin(x)

    def cos(self, x):
        return E(np.cos(x.v), x.a + F) if self.err else np.cos(x)

    def abs(self, x):
        return E(np.abs(x.v), x.a) if self.err else np.abs(x)

    def where(self, c, x, y):
        if self.err:
            x, y = E.lift(x), E.lift(y)
            return E(np.where(c, x.v, y.v), np.where(c, x.a, y.a))
        return np.where(c, x, y)

    def clamp_min(self, x, c):
        """max(x, c) that hands a NaN on"""
        if self.err:
            return E(np.where(x.v < c, c, x.v), np.where(x.v + x.a < c, 0.0, x.a))
        return np.where(x < c, c, x)

    def fmax(self, x, c):
        """max(x, c) that drops a NaN (the clamps of the class term)"""
        if self.err:
            return E(np.fmax(x.v, c), np.where(x.v + x.a < c, 0.0, x.a))
        return np.fmax(x, c)

    def noerr(self, x):
        return E(x.v, 0.0) if self.err else x

    def sl_grad(self, d, beta):
        """d / beta where |d| < beta, else sign(d)"""
        if self.err:
            q = d / beta
            n = np.abs(d.v)
            return E(np.where(n < beta, q.v, np.sign(d.v)), np.where(n < beta + d.a, d.a / beta + U * np.abs(q.v), 0.0))
        return np.where(np.abs(d) < beta, d / beta, np.sign(d))

    def corner_grad(self, D, m):
        """D where m < 1, else D / m"""
        if self.err:
            q = D / m
            quad = m.v < 1.0
            near = np.abs(m.v - 1.0) <= m.a
            return E(np.where(quad, D.v, q.v), np.where(quad, D.a, q.a) + np.where(near, np.abs(D.v) * m.a / np.maximum(m.v, 1e-300), 0.0))
        return np.where(m < 1.0, D, D / m)


def flat2(a, N):
    """(.., W) -> (N, W), N = 0 included"""
    a = np.asarray(a)
    return a.reshape(N, a.shape[-1])


def sigmoid32(x):
    """p of the header in float32, every operation on its own"""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(x))
        r = np.float32(1) / (np.float32(1) + e)
        return np.where(x >= 0, r, e * r)


def _tree8(u):
    """((u_0 + u_4) + (u_2 + u_6)) + ((u_1 + u_5) + (u_3 + u_7)) over the last axis"""
    c = lambda j: u[:, j]
    return ((c(0) + c(4)) + (c(2) + c(6))) + ((c(1) + c(5)) + (c(3) + c(7)))


# ------------------------------------------------------------------------------------------------------------------ the restatement
def restate(d, dt=np.float64, own=False, defect=None, norms_k=None, g=1.0):
    """d: cls (N,), reg (N, 7), rois (N, 7), gt, src (N, W >= 7), mask (N,) int64, labels (N,) float32 or int64, w (dict), corner (bool),
    B (scenes: only the per_scene_norm defect reads it)
    -> dict: out (5), norms (2), d_cls (N,), d_reg (N, 7), the masks, and with dt = "err" the bounds a_out, a_d_cls, a_d_reg"""
    assert defect is None or defect in DEFECTS
    assert not own or dt is np.float64
    O = Ops(dt)
    T = O.T
    c = (lambda v: T(v)) if own else (lambda v: T(np.float32(v)))
    cls32 = np.asarray(d["cls"], np.float32).reshape(-1)
    N = cls32.shape[0]
    labels = np.asarray(d["labels"]).reshape(-1)
    fg = np.asarray(d["mask"]).reshape(-1) > 0
    lab32 = labels.astype(np.float32)
    valid = lab32 >= 0
    if defect == "ignored_as_background":
        valid = np.ones_like(valid)
    corner = bool(d["corner"])
    wq = [float(d["w"]["rcnn_cls_weight"]), float(d["w"]["rcnn_reg_weight"]), float(d["w"]["rcnn_corner_weight"]) if corner else 0.0]
    if not own:
        wq = [f32(v) for v in wq]
    beta, one, half = (T(1.0 / 9.0) if own else T(BETA32)), T(1), T(0.5)
    hx, hy, hz = (h.astype(T)[None] for h in (HX, HY, HZ))
    col = lambda x: x[:, None]
    with np.errstate(all="ignore"):
        # ---- class
        x, t = O.inp(cls32), O.inp(np.maximum(lab32, 0))
        e = O.exp(-O.abs(x))
        r = one / (one + e)
        p = O.where(raw(x) >= 0, r, e * r)
        om = one - p
        l1, l0 = O.fmax(O.log(om), T(-100)), O.fmax(O.log(p), T(-100))
        term_c = (t - one) * l1 - t * l0
        pq = om * p
        dcl = ((p - t) / O.fmax(pq, c(1e-12))) * pq
        sat_hi, sat_lo = sigmoid32(cls32) == 1, cls32 <= -101
        term_c = O.where(sat_hi, T(100) * (one - t), O.where(sat_lo, T(100) * t, term_c))
        dcl = O.where(sat_hi, T(0), O.where(sat_lo, O.noerr(dcl), dcl))
        # ---- regression
        reg, rois = O.inp(flat2(d["reg"], N)), O.inp(flat2(d["rois"], N))
        gt, src = O.inp(flat2(d["gt"], N)[:, :7]), O.inp(flat2(d["src"], N)[:, :7])
        a3, a4, a5 = (O.clamp_min(rois[:, k], c(1e-5)) for k in (3, 4, 5))
        g3, g4, g5 = (O.clamp_min(gt[:, k], c(1e-5)) for k in (3, 4, 5))
        diag = O.sqrt(a3 * a3 + a4 * a4)
        v6 = gt[:, 6] - rois[:, 6] if defect == "heading_not_zeroed" else gt[:, 6]
        v = [gt[:, 0] / diag, gt[:, 1] / diag, gt[:, 2] / a5, O.log(g3 / a3), O.log(g4 / a4), O.log(g5 / a5), v6]
        term_r, gr, live = [], [], []
        for k in range(7):
            dk = reg[:, k] - v[k]
            n = O.abs(dk)
            term_r.append(O.where(raw(n) < beta, half * (n * n) / beta, n - half * beta))
            gr.append(O.sl_grad(dk, beta))
            live.append(~np.isnan(raw(v[k])) & fg)
        # ---- corner
        term_k, cn = None, None
        if corner:
            s3, s4, s5 = (a3, a4, a5) if defect == "clamped_decode" else (rois[:, 3], rois[:, 4], rois[:, 5])
            dg = O.sqrt(s3 * s3 + s4 * s4)
            bx, by, bz = reg[:, 0] * dg, reg[:, 1] * dg, reg[:, 2] * s5
            l = [O.exp(reg[:, 3 + k]) * s for k, s in enumerate((s3, s4, s5))]
            h = reg[:, 6] + rois[:, 6]
            cc, ss = O.cos(rois[:, 6]), O.sin(rois[:, 6])
            cx, cy, cz = (bx * cc - by * ss) + rois[:, 0], (bx * ss + by * cc) + rois[:, 1], bz + rois[:, 2]
            ch, sh = col(O.cos(h)), col(O.sin(h))
            X, Y, Z = col(l[0]) * hx, col(l[1]) * hy, col(l[2]) * hz
            Rx, Ry = X * ch - Y * sh, X * sh + Y * ch
            P = (Rx + col(cx), Ry + col(cy), Z + col(cz))
            gx, gy, gz = col(src[:, 3]) * hx, col(src[:, 4]) * hy, col(src[:, 5]) * hz

            def twin(a):
                cg, sg = col(O.cos(a)), col(O.sin(a))
                Q = ((gx * cg - gy * sg) + col(src[:, 0]), (gx * sg + gy * cg) + col(src[:, 1]), gz + col(src[:, 2]))
                D = [P[i] - Q[i] for i in range(3)]
                return O.sqrt((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]), D
            da, Da = twin(src[:, 6])
            db, Db = twin(src[:, 6] + (T(np.pi) if own else T(PI32)))
            flip = raw(db) < raw(da)
            if defect == "no_twin":
                flip = np.zeros_like(flip)
            m = O.where(flip, db, da)
            D = [O.where(flip, Db[i], Da[i]) for i in range(3)]
            if defect == "corner_beta_ninth":
                sl = O.where(raw(m) < beta, half * (m * m) / beta, m - half * beta)
                G = [O.where(raw(m) < beta, D[i] / beta, D[i] / m) for i in range(3)]
            else:
                sl = O.where(raw(m) < 1.0, (half * m) * m, m - half)
                G = [O.corner_grad(D[i], m) for i in range(3)]
            term_k = T(0.125) * sl                                                   # (N, 8)
            qx, qy = G[0] * ch + G[1] * sh, G[1] * ch - G[0] * sh
            Uc = [_tree8(u) for u in (G[0], G[1], G[2], qx * hx, qy * hy, G[2] * hz, G[1] * Rx - G[0] * Ry)]
            ex, ey = Uc[0] * cc + Uc[1] * ss, Uc[1] * cc - Uc[0] * ss
            cn = [ex * dg, ey * dg, Uc[2] * s5, Uc[3] * l[0], Uc[4] * l[1], Uc[5] * l[2], Uc[6]]
            ties = np.where(col(fg), np.abs(raw(da) - raw(db)), np.inf)
    # ---- sums: float64, then the header's double expression
    scenes = np.arange(N) // max(N // max(int(d.get("B", 1)), 1), 1) if defect == "per_scene_norm" else np.zeros(N, np.int64)
    nsc = int(scenes.max()) + 1 if N else 1
    cnt = lambda msk: np.maximum(np.bincount(scenes[msk], minlength=nsc), 1).astype(np.float64)
    nv, nf = cnt(valid), cnt(fg)
    if defect == "reg_by_valid":
        nf = nv
    masked = [(term_c, valid)] + [(term_r[k], live[k]) for k in range(7)] + ([(term_k, col(fg) & np.ones((1, 8), bool))] if corner else [])
    quantity = [0] + [1] * 7 + [2]
    out, t_abs, a_sum = np.zeros(3), np.zeros(3), np.zeros(3)
    for (term, msk), q in zip(masked, quantity):
        n_of = (nv if q == 0 else nf)[scenes]
        scale = wq[q] / (n_of if msk.ndim == 1 else n_of[:, None]) / nsc
        val = np.where(msk, wide(raw(term)), 0.0)
        out[q] += (val * scale).sum()
        t_abs[q] += (np.abs(val) * np.abs(scale)).sum()
        if O.err:
            a_sum[q] += (np.where(msk, term.a, 0.0) * np.abs(scale)).sum()
    norms = np.array([1.0 / nv[0], 1.0 / nf[0]])
    R = dict(N=N, valid=valid, fg=fg, sat_hi=sat_hi & valid, sat_lo=sat_lo & valid, live=np.stack(live, 1) if N else np.zeros((0, 7), bool),
             ties=ties if corner else None, m=raw(m) if corner else None)
    if T is np.float32:
        o = out.astype(np.float32)
        o3 = o[1] + o[2]
        out = np.array([o[0], o[1], o[2], o3, o[0] + o3], np.float32)
        norms = norms.astype(np.float32)
    else:
        o3 = out[1] + out[2]
        out = np.array([out[0], out[1], out[2], o3, out[0] + o3])
    R.update(out=out, norms=norms)
    if O.err:
        R["a_out"] = np.array([sum_bound(out[q], t_abs[q], K * a_sum[q]) for q in range(3)])
    # ---- gradients from the kernel's norms (its own when none are given)
    nk = np.asarray(norms_k, np.float32) if norms_k is not None else np.asarray(norms)
    n0, n1 = (1.0 / nv[scenes] / nsc, 1.0 / nf[scenes] / nsc) if defect == "per_scene_norm" else (nk[0], nk[1])
    if defect == "reg_by_valid" and norms_k is None:
        n1 = nk[0]
    lift = (lambda s: E(np.asarray(s, np.float64))) if O.err else (lambda s: np.asarray(s).astype(T))
    with np.errstate(all="ignore"):
        if own:
            gv, gf = T(g) * lift(n0), T(g) * lift(n1)
        else:
            gv, gf = lift(np.float32(g)) * lift(n0), lift(np.float32(g)) * lift(n1)
        s0, s1, s2 = gv * T(wq[0]), gf * T(wq[1]), (gf * T(wq[2])) * T(0.125)
        d_cls = O.where(valid, s0 * dcl, T(0))
        cols = []
        for k in range(7):
            part = O.where(live[k], s1 * gr[k], T(0))
            if corner:
                part = part + s2 * cn[k]
            cols.append(O.where(fg, part, T(0)))
    R["d_cls"] = raw(d_cls)
    R["d_reg"] = np.stack([raw(x) for x in cols], 1) if N else np.zeros((0, 7), T)
    if O.err:
        R["a_d_cls"] = K * d_cls.a + TINY
        R["a_d_reg"] = K * np.stack([x.a for x in cols], 1) + TINY if N else np.zeros((0, 7))
    return R


def bounds(d, norms_k=None, g=1.0):
    """-> (dict of (ref, bound) per checked stage, the restatement they come from)"""
    R = restate(d, "err", norms_k=norms_k, g=g)
    out = {name: (R["out"][q:q + 1], R["a_out"][q:q + 1]) for q, name in enumerate(("out_cls", "out_reg", "out_corner"))}
    out["d_cls"], out["d_reg"] = (R["d_cls"], R["a_d_cls"]), (R["d_reg"], R["a_d_reg"])
    return out, R


def seam_expected(d, norms_k, g):
    """without the corner term: columns 2 and 6 of foreground rois whose float32 difference has n >= beta: (mask, the exact float32 d_reg)"""
    N = np.asarray(d["mask"]).size
    reg, rois, gt = (flat2(d[k], N).astype(np.float32) for k in ("reg", "rois", "gt"))
    with np.errstate(all="ignore"):
        a5 = np.where(rois[:, 5] < np.float32(1e-5), np.float32(1e-5), rois[:, 5])
        dd = np.zeros((N, 7), np.float32)
        dd[:, 2], dd[:, 6] = reg[:, 2] - gt[:, 2] / a5, reg[:, 6] - gt[:, 6]
        mask = (np.asarray(d["mask"]).reshape(-1) > 0)[:, None] & (np.abs(dd) >= BETA32) & (not bool(d["corner"]))
        mask[:, [0, 1, 3, 4, 5]] = False
        s1 = (np.float32(g) * np.asarray(norms_k, np.float32)[1]) * np.float32(d["w"]["rcnn_reg_weight"])
        want = (s1 * np.sign(dd)).astype(np.float32)
    return mask, want


def check_roi(W, d, got, where=""):
    """got: out (5), norms (2), d_cls (N,), d_reg (N, 7), g (the upstream gradient the backward ran with) -- float32"""
    bd, R = bounds(d, norms_k=got["norms"], g=got["g"])
    o = np.asarray(got["out"], np.float32)
    d_cls, d_reg = np.asarray(got["d_cls"], np.float32).reshape(-1), np.asarray(got["d_reg"], np.float32).reshape(-1, 7)
    for q, name in enumerate(("out_cls", "out_reg", "out_corner")):
        W.check(name, o[q:q + 1], bd[name], where)
    W.exact("out_regsum", o[3], o[1] + o[2], where)
    W.exact("out_total", o[4], o[0] + o[3], where)
    nv, nf = max(int(R["valid"].sum()), 1), max(int(R["fg"].sum()), 1)
    W.exact("norms", np.asarray(got["norms"], np.float32), np.array([1.0 / nv, 1.0 / nf]).astype(np.float32), where)
    W.check("d_cls", d_cls, bd["d_cls"], where)
    W.check("d_reg", d_reg, bd["d_reg"], where)
    W.require(not np.any(d_cls[~R["valid"]]), f"{where}: d_cls at an ignored roi")
    W.require(not np.any(d_reg[~R["fg"]]), f"{where}: d_reg at a non-foreground roi")
    W.exact("sat", d_cls[R["sat_hi"]], np.zeros(int(R["sat_hi"].sum()), np.float32), where)
    if not d["corner"]:
        W.require(float(o[2]) == 0.0, f"{where}: a corner term without with_corner")
    if not R["fg"].any():
        W.require(float(o[1]) == 0.0 and float(o[2]) == 0.0, f"{where}: no foreground roi")
    mask, want = seam_expected(d, got["norms"], got["g"])
    W.exact("seam", d_reg[mask], want[mask], where)
    W.require(np.isfinite(o).all() and np.isfinite(got["norms"]).all(), where)


def emulate(d, defect=None, g=G_UP):
    """the float32 emulation of both launches, in the shape check_roi takes"""
    R = restate(d, dt=np.float32, defect=defect, g=g)
    return dict(out=R["out"], norms=R["norms"], d_cls=R["d_cls"], d_reg=R["d_reg"], g=g)


# ------------------------------------------------------------------------------------------------------------------ margins
TIE_MARGIN = 1e-3


def margins(d):
    """what the cases are built around, measured in float64 over what the labels and the mask include:
    tie    the smallest |dist(Q) - dist(Q')| over foreground corners (inf without the corner term)
    one    the smallest |m - 1| over foreground corners
    beta   the smallest | |r_k - v_k| - beta | over live columns whose target is COMPUTED (0, 1, 3, 4, 5)
    trig   the largest |argument| handed to sinf / cosf
    logit  True when every valid logit lies in [-20, 10], at or above 17, or at or below -101"""
    R = restate(d)
    N = R["N"]
    fg, valid = R["fg"], R["valid"]
    reg, rois, src = (flat2(d[k], N).astype(np.float64) for k in ("reg", "rois", "src"))
    out = dict(tie=np.inf, one=np.inf, trig=0.0)
    if d["corner"] and fg.any():
        out["tie"] = float(R["ties"][fg].min())
        out["one"] = float(np.abs(R["m"][fg] - 1.0).min())
        out["trig"] = float(np.max(np.abs(np.stack([rois[fg, 6], reg[fg, 6] + rois[fg, 6], src[fg, 6], src[fg, 6] + np.pi]))))
    x = np.asarray(d["cls"], np.float64).reshape(-1)[valid]
    out["logit"] = bool(np.all(((x >= -20) & (x <= 10)) | (x >= 17) | (x <= -101)))
    return out


def assert_margins(d):
    m = margins(d)
    assert m["tie"] > TIE_MARGIN, "two corner distances within %g of each other (%g)" % (TIE_MARGIN, m["tie"])
    assert m["trig"] <= 2 * np.pi, "a trig argument outside [-2 pi, 2 pi] (%g)" % m["trig"]
    assert m["logit"], "a valid logit where a float32 1 - p has few correct digits"
    return m


# ------------------------------------------------------------------------------------------------------------------ case lists
SHAPE_N = [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3]
# one sweep of the capped grid covers MAX_TILES * TILE rois: one below, at, above
CAP = MAX_TILES * TILE
CAP_N = [CAP - 1, CAP, CAP + 1]
VALUE_KINDS = ["no_fg", "no_valid", "all_fg", "fg_ignored", "dist_zero", "dist_one", "beta_seam", "twin_nearer", "tiny_dims", "heading_out",
               "logit_sat", "nan_target", "labels_i64"]
LOGIT_EDGES = [17.0, 20.0, 120.0, -104.0, 0.0, -20.0, 10.0, -10.0]
DIST_EDGES = [0.9, 0.999, 1.001, 1.1, 0.5, 2.0]
TINY_DIMS = [0.0, 1e-6, 9e-6, 1e-5, 2e-5]
HEADINGS_OUT = [-2.5, 4.0, 5.5, -4.0]
VALUE_N = 2 * 67


def shape_cases():
    return [dict(N=N, kind="random", labels=lab, corner=cor) for N in SHAPE_N for (lab, cor) in (("roi_iou", True), ("cls", False))]


def cap_cases():
    return [dict(N=N, kind="random", labels="roi_iou", corner=True) for N in CAP_N]


def value_cases():
    return [dict(N=VALUE_N, kind=kind, labels=("cls" if kind in ("no_valid", "fg_ignored", "labels_i64") else "roi_iou"), corner=cor)
            for kind in VALUE_KINDS for cor in (True, False)]


KITTI_CASE = dict(N=256, kind="random", labels="roi_iou", corner=True)
LARGE_CASE = dict(N=300001, kind="random", labels="cls", corner=True)


def case_name(c):
    return "-".join(str(v) for v in c.values())


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def canonical(rois, src):
    """gt_of_rois from gt_of_rois_src as canonical_targets forms it (float32 numpy; an INPUT of the loss, not checked here)"""
    f = np.float32
    ry = np.mod(rois[:, 6], f(2 * np.pi))
    loc = src[:, 0:3] - rois[:, 0:3]
    cs, sn = np.cos(-ry), np.sin(-ry)
    x, y = loc[:, 0] * cs - loc[:, 1] * sn, loc[:, 0] * sn + loc[:, 1] * cs
    hd = np.mod(src[:, 6] - ry, f(2 * np.pi))
    opp = (hd > f(np.pi / 2)) & (hd < f(3 * np.pi / 2))
    hd = np.where(opp, np.mod(hd + f(np.pi), f(2 * np.pi)), hd)
    hd = np.where(hd > f(np.pi), hd - f(2 * np.pi), hd)
    hd = np.clip(hd, f(-np.pi / 2), f(np.pi / 2))
    return np.stack([x, y, loc[:, 2], src[:, 3], src[:, 4], src[:, 5], hd, src[:, 7]], 1).astype(f)


def make_case(c, poison=True):
    """seeded inputs of one case; poison: what the labels and the mask exclude holds NaN, else zeros"""
    N, kind, cor = c["N"], c["kind"], c["corner"]
    rng = np.random.default_rng(_seed("roi_loss", *c.values()))
    f = np.float32
    small = kind == "tiny_dims"
    rois = np.concatenate([rng.uniform(-1, 1, (N, 3)) if small else rng.uniform(-10, 10, (N, 3)), rng.uniform(0.5, 4.0, (N, 3)), rng.uniform(-3, 3, (N, 1))], 1).astype(f)
    src = np.concatenate([rois[:, 0:3] + rng.standard_normal((N, 3)) * 0.3, rois[:, 3:6] * np.exp(rng.standard_normal((N, 3)) * 0.1),
                          np.clip(rois[:, 6:7] + rng.standard_normal((N, 1)) * 0.2, -3.1, 3.1), np.ones((N, 1))], 1).astype(f)
    reg = np.concatenate([rng.standard_normal((N, 3)) * 0.15, rng.standard_normal((N, 3)) * 0.1, np.clip(rng.standard_normal((N, 1)) * 0.2, -1, 1)], 1).astype(f)
    cls = np.clip(rng.standard_normal(N) * 2.5, -8, 8).astype(f)
    mask = (rng.random(N) < 0.3).astype(np.int64)
    k = np.arange(N)
    if c["labels"] == "cls":
        u = rng.random(N)
        labels = np.where(u < 0.2, -1, np.where(u < 0.6, 1, 0)).astype(np.int64)
    else:
        labels = np.where(k % 5 == 0, 0.0, np.where(k % 5 == 1, 1.0, rng.random(N))).astype(f)
    if kind == "no_fg":
        mask[:] = 0
    elif kind == "no_valid":
        labels[:] = -1
    elif kind == "all_fg":
        mask[:] = 1
    elif kind == "fg_ignored":
        mask[::2] = 1
        labels[::4] = -1
    elif kind in ("dist_zero", "dist_one"):       # reg = 0 decodes to the roi itself; the matched box is the roi, moved along z
        mask[::2] = 1
        reg[::2] = 0
        src[::2, :7] = rois[::2]
        if kind == "dist_one":
            src[::2, 2] += np.array(DIST_EDGES, f)[(k[::2] // 2) % len(DIST_EDGES)]
    elif kind == "beta_seam":                     # gt_2 = gt_6 = 0: d = r_2, r_6 exactly; 0, +-beta, its float32 neighbours, +-0.6
        up, dn = np.nextafter(BETA32, f(1)), np.nextafter(BETA32, f(0))
        edges = np.array([0.0, BETA32, -BETA32, up, -up, dn, -dn, 0.6, -0.6], f)
        mask[::2] = 1
        reg[:, 2], reg[:, 6] = edges[k % 9], edges[(k // 2 + 3) % 9]
    elif kind == "twin_nearer":
        mask[::2] = 1
        turned = src[::2, 6] + f(np.pi)
        src[::2, 6] = np.where(turned > 3.1, turned - f(2 * np.pi), turned)
    elif kind == "tiny_dims":
        mask[::2] = 1
        td = np.array(TINY_DIMS, f)
        rois[::6, 3], rois[2::6, 4], rois[4::6, 5] = td[(k[::6] // 6) % 5], td[(k[2::6] // 6) % 5], td[(k[4::6] // 6) % 5]
        rois[12::24, 3:6] = 0
    elif kind == "heading_out":
        mask[::2] = 1
        rois[::2, 6] = np.array(HEADINGS_OUT, f)[(k[::2] // 2) % len(HEADINGS_OUT)]
        reg[::2, 6] = np.clip(reg[::2, 6], -0.5, 0.5)
        wrapped = np.mod(rois[::2, 6] + np.pi, 2 * np.pi) - np.pi
        src[::2, 6] = np.clip(wrapped + rng.standard_normal(wrapped.shape) * 0.2, -3.1, 3.1).astype(f)
    elif kind == "logit_sat":
        cls = np.array(LOGIT_EDGES, f)[(k + int(rng.integers(0, 8))) % len(LOGIT_EDGES)]
        labels = np.array([0.0, 1.0, 0.25, 0.5, 1.0, 0.0, 0.75], f)[(k // 3) % 7]
    gt = canonical(rois, src)
    if kind == "beta_seam":
        gt[:, 2], gt[:, 6] = 0, 0
    elif kind == "tiny_dims":
        gt[::14, 3:6] = np.array(TINY_DIMS, f)[(k[::14] // 14) % 5][:, None]
    elif kind == "nan_target":
        mask[::2] = 1
        hole = rng.random((N, 8)) < 0.2
        hole[:, [4, 5, 7]] = False
        gt[hole] = np.nan
    if cor:                                        # move the few foreground rois whose two corner distances nearly tie
        d0 = dict(cls=cls, reg=reg, rois=rois, gt=gt, src=src, mask=mask, labels=labels, w=dict(W_DEFAULT), corner=True, B=2)
        for _ in range(6):
            ties = restate(d0)["ties"].min(1) if N else np.zeros(0)
            near = ties <= 2 * TIE_MARGIN
            if not near.any():
                break
            src[near, 6] = np.clip(src[near, 6] + f(0.07), -3.1, 3.1)
    d = dict(cls=cls, reg=reg, rois=rois, gt=gt, src=src, mask=mask, labels=labels, w=dict(W_DEFAULT), corner=cor, B=2 if N % 2 == 0 and N else 1)
    assert_margins(d)
    bad = f(np.nan) if poison else f(0)
    ign, off = labels < 0, mask <= 0
    d["cls"][ign] = bad
    d["reg"][off], d["rois"][off], d["gt"][off], d["src"][off] = bad, bad, bad, bad
    return d


def kind_of(d):
    return KIND_CLS if np.asarray(d["labels"]).dtype == np.int64 else KIND_ROI_IOU


def gold():
    g = np.load(GOLD)
    return g, json.loads(str(g["cases"]))


def gold_case(g, name, corner=True):
    """the recorded inputs of a golden case as a case dict"""
    B = int(g[name + "/rois"].shape[0])
    return dict(cls=g[name + "/cls"], reg=g[name + "/reg"], rois=g[name + "/rois"].reshape(-1, 7), gt=g[name + "/gt"].reshape(-1, 8),
                src=g[name + "/src"].reshape(-1, 8), mask=g[name + "/mask"].astype(np.int64).reshape(-1), labels=g[name + "/labels"].reshape(-1),
                w=dict(W_DEFAULT), corner=corner, B=B)
