"""Float64 reference of the kernels that make the training loss and apply the update -- csrc/occ_loss.hip, btc_occ_prob and
btc_sumsq2_* of csrc/glue.hip, csrc/optim.hip -- stage by stage, with a derived error bound for every stage, the inputs of the
shared case lists and the checks both test modules run.  Plain numpy: no GPU, no autograd.  The conventions are those of
tests/bn_ref.py: every function returns (reference, bound), `ratio` above 1 is a failure, float arguments are float64(float32(v)),
bfloat16 widens exactly, and a stage that consumes an earlier result takes the KERNEL's value of it (the per-quantity sums for
out / norms, the norms for the gradients, total_sq for the Adam update).

Notation: u = 2^-24 (one correctly rounded fp32 operation, relative).  The library is built with -ffp-contract=off, so every fp32
operation of the kernels rounds on its own; + - * / are correctly rounded (hipcc's default for fp32 division).  Neither the ROCm
headers nor its documentation state an accuracy for the device's expf / logf / sqrtf and nobody has measured it here: 2 ulp = 4 u
is ASSUMED for the three (F below); expf(0) = 1 exactly.  A subnormal expf result may be flushed: 2^-125 absolute (FLOOR) on each
softmax value.  Every elementwise bound is K = 2 times the first-order count written below (twice, the factor bn_ref.py takes); a
cross-cell sum is accumulated in float64 and rounded once: 2^-23 |ref| + 2^-40 sum|terms| plus the sum of the per-term bounds.  The
sums that are read back as float64 (the occupancy loss's per-block partials, Adam's total_sq) were never rounded to fp32 and go
without the 2^-23 |ref|; their longest chain of float64 additions is a few hundred, 2^-44 sum|terms| at the very worst.

softmax.  delta = |z1 - z0|, e = exp(-delta) for the smaller logit (one rounding of the argument: delta u relative on e, plus F),
1 for the larger.  inv = 1 / (e0 + e1), s_t = e_t inv: three roundings.  With s_o the other class,
    A_s(t) = s_t (3 u + (delta + 4) u s_o) + FLOOR              (d s_t / s_t = +- s_o d e / e for either class)
occ loss, per cell.  p = s_t + eps, om = 1 - p, L = logf(p), FL = -(om om) L:
    A_p = A_s + u p,   A_om = A_p + u |om|,   A_L = A_p / p + F |L|
    A_FL = 2 |om| |L| A_om + om^2 A_p / p + (2 u + F) |FL|
  the first two terms are |dFL/dp| A_p: ABSOLUTE 2^-24-sized errors on p that matter where om is about 1e-6 (p within eps of 1).
smooth L1, per component.  d = |res - tgt| (u d), then 0.5 d d / beta (two more roundings) or d - 0.5 beta (one):
    A_SL = 4 u SL   (|d| < beta),      u (d + SL)   (otherwise)
  at |d| = beta both branches give beta / 2, so a comparison decided the other way by the rounding of d costs u beta, inside both.
sums S0 = sum w_c FL, S1 = sum w_c, S2 = sum w_r (SL_0 + SL_1 + SL_2), S3 = sum w_r (float64 in the kernel; read from its per-block
partials): K sum w A + 2^-40 sum|terms|.
out[0] = S0_k / max(S1_k, 1) w_cls, out[1] likewise, norms[i] = w / max(S_k, 1): one rounding to fp32, 2^-23 |ref|.
out[2] = fp32(out[0] + out[1]) of the kernel's own two values: bit-exact.
d_logit.  dfdp = T1 - T2, T1 = 2 om L, T2 = om om / p:
    A_T1 = 2 |L| A_om + 2 |om| A_L + u |T1|,    A_T2 = 2 |om| A_om / p + om^2 A_p / p^2 + 2 u |T2|,    A_df = A_T1 + A_T2 + u |dfdp|
    scale = g norms_k[0] w_c dfdp (c = g n w):  A_sc = |c| A_df + 3 u |scale|
    d z_t = scale s_t (1 - s_t):   A = A_sc s_t s_o + |scale| (A_s(t) s_o + s_t (A_s(t) + u s_o)) + 2 u |ref|
    d z_o = -scale s_t s_o:        A = A_sc s_t s_o + |scale| (A_s(t) s_o + s_t A_s(o)) + 2 u |ref|
d_res = (g norms_k[1] w_r) gr, gr = d / beta or sign(d): at most five roundings, A = 5 u |ref|.
occ_prob = e1 / (e0 + e1) mask: A = s_1 (2 u + (delta + 4) u s_0) + FLOOR.
sumsq2 forward.  16-byte vectors of 4 fp32 / 8 bf16 values are squared and added in fp32 (bf16 squares are exact), at most four
roundings on a vector's sum, then everything is float64: 2^-23 |ref| + 2^-40 T + 2^-21 T, T = |ka| sum a^2 + |kb| sum b^2
(2^-21 = 8 u, twice the count).  sumsq2 backward: da = a fp32(g ka2), for bf16 a bf16(a bf16(fp32(g ka2))): bit-exact in numpy.
adam.  total_sq (float64 sum of exact products): 2^-40 sum g^2.  Per element, from the kernel's total_sq:
    inv_coef = max((fp32(sqrt(tsq)) + 1e-6) / clip, 1): 3 u;  gr = g / inv_coef:  r = 4 u (clip on), 0 (clip off: g / 1)
    m' = m + c1 (gr - m), c1 = 1 - b1:    A_m = c1 r |gr| + 3 u c1 |gr - m| + u |m'|
    v' = b2 v + (c2 gr) gr, c2 = 1 - b2:  A_v = u b2 v + (3 u + 2 r) c2 gr^2 + u v'
    den = sqrtf(v') isb + eps:            A_den = sqrt(v') isb (A_v / (2 v') + F + 2 u) + u den     (isb = fp32(1 / sqrt(bc2)))
    upd = lob m' / den:                   A_upd = |upd| (3 u + A_den / den) + lob A_m / den           (lob = fp32(lr / bc1))
    p' = p decay - upd:                   A_p = 3 u |p decay| + A_upd + u |p'|                        (decay = fp32(1 - fp32(wd lr)))
grads_pack: a copy, bit-exact.

tests/test_loss_ref_cpu.py ties these formulas to torch float64 (autograd, clip_grad_norm_ + torch.optim.Adam, one-liners) at 1e-12,
runs a numpy fp32 emulation of every kernel (same grids, grid strides, summation orders, chunk and launch loops) over the case
lists below, and shows for thirteen seeded defects that some case exceeds its bound.  Worst ratio |got - ref| / bound of that
emulation per stage, over all cases:

  S 0.252   out 0.485   norms 0.413   d_logit 0.215   d_res 0.309   occ_prob 0.345   sumsq2_fwd 0.113   total_sq 0.001
  adam_p 0.277   adam_m 0.471   adam_v 0.489          bit-exact (out_total, sumsq2_bwd, grads_pack): equal in every case
"""
import zlib

import numpy as np

from bn_ref import TINY, bf16_round, f32, ratio, wide

U = 2.0 ** -24
F = 4.0 * U          # expf / logf / sqrtf: 2 ulp, assumed
FLOOR = 2.0 ** -125
K = 2.0
EPS = f32(1e-6)
BETA, W_CLS, W_RES, G_UP = 0.11, 1.0, 0.1, 0.7
ADAM_MAX_SEGMENTS = 448

STAGES = ("S", "out", "norms", "out_total", "d_logit", "d_res", "occ_prob", "sumsq2_fwd", "sumsq2_bwd", "total_sq", "adam_p", "adam_m",
          "adam_v", "grads_pack")
EXACT = ("out_total", "sumsq2_bwd", "grads_pack")


def sum_bound(ref, terms_abs_sum, per_term=0.0, rounded=True):
    """a float64 accumulation; rounded: the result is then rounded to fp32 once"""
    return (2.0 ** -23 if rounded else 0.0) * np.abs(ref) + 2.0 ** -40 * terms_abs_sum + per_term + TINY


# ------------------------------------------------------------------------------------------------------------------ occupancy loss
def _softmax2(z0, z1):
    """-> s0, s1, delta in float64 (exp of a non-positive argument only)"""
    delta = np.abs(z1 - z0)
    e = np.exp(-delta)
    lo, hi = e / (1.0 + e), 1.0 / (1.0 + e)
    up = z1 >= z0
    return np.where(up, lo, hi), np.where(up, hi, lo), delta


def _a_s(st, so, delta):
    return st * (3 * U + (delta + 4.0) * U * so) + FLOOR


def _cls_cells(d):
    """cells inside cls_mask: flat index, s_t, s_o, delta, pos"""
    B, _, n = d["logit"].shape
    idx = np.flatnonzero(d["cm"].reshape(-1))
    b, sp = idx // n, idx % n
    z0, z1 = wide(d["logit"][b, 0, sp]), wide(d["logit"][b, 1, sp])
    s0, s1, delta = _softmax2(z0, z1)
    pos = d["pos"].reshape(-1)[idx] != 0
    return idx, b, sp, np.where(pos, s1, s0), np.where(pos, s0, s1), delta, pos


def _focal(st, so, delta, eps=EPS):
    """-> p, om, L, FL and the first-order errors A_p, A_om, A_L, A_FL"""
    p = st + eps
    om = 1.0 - p
    L = np.log(p)
    FL = -(om * om) * L
    a_p = _a_s(st, so, delta) + U * p
    a_om = a_p + U * np.abs(om)
    a_L = a_p / p + F * np.abs(L)
    a_FL = 2 * np.abs(om * L) * a_om + om * om * a_p / p + (2 * U + F) * np.abs(FL)
    return p, om, L, FL, a_p, a_om, a_L, a_FL


def _reg_cells(d):
    """cells inside reg_mask (none without a residual head): flat index, b, sp, signed d (3, cells)"""
    if d["res"] is None:
        e = np.zeros(0, dtype=np.int64)
        return e, e, e, np.zeros((3, 0))
    n = d["res"].shape[2]
    idx = np.flatnonzero(d["rm"].reshape(-1))
    b, sp = idx // n, idx % n
    dd = np.stack([wide(d["res"][b, k, sp]) - wide(d["tgt"][b, k, sp]) for k in range(3)])
    return idx, b, sp, dd


def occ_sums(d, eps=EPS):
    """-> (S[4], bound[4]); eps: the kernel's float32(1e-6) unless a formula check aligns it with another implementation's"""
    beta = f32(d["beta"])
    idx, _, _, st, so, delta, _ = _cls_cells(d)
    w = wide(d["cw"].reshape(-1)[idx])
    foc = _focal(st, so, delta, eps)
    FL, a_FL = foc[3], foc[7]
    S = np.zeros(4)
    Bd = np.zeros(4)
    S[0], S[1] = (w * FL).sum(), w.sum()
    Bd[0] = sum_bound(S[0], np.abs(w * FL).sum(), K * (np.abs(w) * a_FL).sum(), False)
    Bd[1] = sum_bound(S[1], np.abs(w).sum(), 0.0, False)
    ridx, _, _, dd = _reg_cells(d)
    wr = wide(d["rw"].reshape(-1)[ridx]) if ridx.size else np.zeros(0)
    ad = np.abs(dd)
    quad = ad < beta
    SL = np.where(quad, 0.5 * ad * ad / beta, ad - 0.5 * beta)
    a_SL = np.where(quad, 4 * U * SL, U * (ad + SL))
    S[2], S[3] = (wr * SL.sum(0)).sum(), wr.sum()
    Bd[2] = sum_bound(S[2], np.abs(wr * SL.sum(0)).sum(), K * (np.abs(wr) * a_SL.sum(0)).sum(), False)
    Bd[3] = sum_bound(S[3], np.abs(wr).sum(), 0.0, False)
    return S, Bd


def occ_out(d, S_k):
    """from the kernel's sums -> (out[0:2], bound), (norms, bound)"""
    S_k = wide(S_k)
    nc, nr = max(S_k[1], 1.0), max(S_k[3], 1.0)
    out = np.array([S_k[0] / nc * f32(d["w_cls"]), S_k[2] / nr * f32(d["w_res"])])
    norms = np.array([f32(d["w_cls"]) / nc, f32(d["w_res"]) / nr])
    return (out, 2.0 ** -23 * np.abs(out) + TINY), (norms, 2.0 ** -23 * np.abs(norms) + TINY)


def occ_bwd(d, norms_k, g, eps=EPS):
    """g = (g_cls, g_reg) upstream gradients -> (d_logit, bound), (d_res or None, bound)"""
    beta = f32(d["beta"])
    norms_k = wide(norms_k)
    B, _, n = d["logit"].shape
    dl, bl = np.zeros((B, 2, n)), np.full((B, 2, n), TINY)
    idx, b, sp, st, so, delta, pos = _cls_cells(d)
    p, om, L, _, a_p, a_om, a_L, _ = _focal(st, so, delta, eps)
    T1, T2 = 2 * om * L, om * om / p
    df = T1 - T2
    a_df = (2 * np.abs(L) * a_om + 2 * np.abs(om) * a_L + U * np.abs(T1)) + (2 * np.abs(om) * a_om / p + om * om * a_p / (p * p) + 2 * U * np.abs(T2)) \
        + U * np.abs(df)
    c = f32(g[0]) * norms_k[0] * wide(d["cw"].reshape(-1)[idx])
    scale = c * df
    a_sc = np.abs(c) * a_df + 3 * U * np.abs(scale)
    a_st, a_so = _a_s(st, so, delta), _a_s(so, st, delta)
    dt, do = scale * st * so, -scale * st * so
    a_dt = a_sc * st * so + np.abs(scale) * (a_st * so + st * (a_st + U * so)) + 2 * U * np.abs(dt)
    a_do = a_sc * st * so + np.abs(scale) * (a_st * so + st * a_so) + 2 * U * np.abs(do)
    ct = pos.astype(np.int64)
    dl[b, ct, sp], dl[b, 1 - ct, sp] = dt, do
    bl[b, ct, sp], bl[b, 1 - ct, sp] = K * a_dt + TINY, K * a_do + TINY
    if d["res"] is None:
        return (dl, bl), (None, None)
    dr, br = np.zeros((B, 3, n)), np.full((B, 3, n), TINY)
    ridx, rb, rsp, dd = _reg_cells(d)
    sc = f32(g[1]) * norms_k[1] * wide(d["rw"].reshape(-1)[ridx])
    gr = np.where(np.abs(dd) < beta, dd / beta, np.sign(dd))
    for k in range(3):
        dr[rb, k, rsp] = sc * gr[k]
        br[rb, k, rsp] = K * 5 * U * np.abs(sc * gr[k]) + TINY
    return (dl, bl), (dr, br)


def occ_prob(logit, mask):
    s0, s1, delta = _softmax2(wide(logit[:, 0]), wide(logit[:, 1]))
    m = wide(mask)
    return s1 * m, K * (s1 * (2 * U + (delta + 4.0) * U * s0) + FLOOR) * m + TINY


# ------------------------------------------------------------------------------------------------------------------ sumsq2
def sumsq2_fwd(a, ka, b, kb):
    """a, b: float32 values (bf16 already widened; b None: absent); ka, kb doubles"""
    ta = abs(ka) * float((wide(a) ** 2).sum())
    tb = abs(kb) * float((wide(b) ** 2).sum()) if b is not None else 0.0
    ref = np.array([np.sign(ka) * ta + np.sign(kb) * tb])
    return ref, sum_bound(ref, ta + tb, 2.0 ** -21 * (ta + tb))


def sumsq2_bwd(x, bf, g, k2):
    """bit-exact: x * fp32(g * k2) in fp32; bf16: bf16(x * bf16(fp32(g k2))), as float32 values"""
    s = np.float32(g) * np.float32(k2)
    x = np.ascontiguousarray(x, dtype=np.float32)
    return bf16_round(x * bf16_round(np.array([s]))[0]) if bf else x * s


# ------------------------------------------------------------------------------------------------------------------ adam
def chunk_tables_np(sizes, max_seg=ADAM_MAX_SEGMENTS):
    """train_step.chunk_tables without a device"""
    off, seg, coff, clen, cflat, seg0 = 0, [], [], [], [], [0]
    for i, n in enumerate(sizes):
        for c0 in range(0, n, 1024):
            seg.append(i % max_seg); coff.append(c0); clen.append(min(1024, n - c0)); cflat.append(off + c0)
        seg0.append(len(seg))
        off += n
    return dict(seg=np.array(seg, np.int32), off=np.array(coff, np.int32), len=np.array(clen, np.int32), flat=np.array(cflat, np.int64), seg0=seg0)


def total_sq(gflat):
    g2 = wide(gflat) ** 2
    ref = np.array([g2.sum()])
    return ref, sum_bound(ref, g2.sum(), 0.0, False)


def adam(gflat, p0, m0, v0, tsq_k, hp):
    """hp: step, lr, beta1, beta2, eps, wd, clip -> dict p / m / v: (ref, bound)"""
    g, p0, m0, v0 = wide(gflat), wide(p0), wide(m0), wide(v0)
    lr, b1, b2, eps, wd, clip = (f32(hp[k]) for k in ("lr", "beta1", "beta2", "eps", "wd", "clip"))
    bc1, bc2 = 1.0 - b1 ** hp["step"], 1.0 - b2 ** hp["step"]
    r = 0.0
    if clip > 0:
        g = g / max((np.sqrt(float(tsq_k)) + hp.get("clip_eps", EPS)) / clip, 1.0)
        r = 4 * U
    c1, c2 = 1.0 - b1, 1.0 - b2
    pd = p0 * (1.0 - wd * lr)
    m = m0 + c1 * (g - m0)
    v = b2 * v0 + c2 * g * g
    a_m = c1 * r * np.abs(g) + 3 * U * c1 * np.abs(g - m0) + U * np.abs(m)
    a_v = U * b2 * v0 + (3 * U + 2 * r) * c2 * g * g + U * v
    isb, lob = 1.0 / np.sqrt(bc2), lr / bc1
    sq = np.sqrt(v)
    den = sq * isb + eps
    a_den = isb * (a_v / (2 * np.where(sq > 0, sq, 1.0)) + sq * (F + 2 * U)) + U * den
    upd = lob * m / den
    a_upd = np.abs(upd) * (3 * U + a_den / den) + lob * a_m / den
    p = pd - upd
    a_p = 3 * U * np.abs(pd) + a_upd + U * np.abs(p)
    return dict(p=(p, K * a_p + TINY), m=(m, K * a_m + TINY), v=(v, K * a_v + TINY))


# ------------------------------------------------------------------------------------------------------------------ case lists
OCC_SMALL = [(1, 1), (1, 63), (1, 255), (1, 256), (1, 257), (3, 257), (1, 2048), (1, 2049)]
OCC_LARGE = [(2, 65 * 1024 + 5), (1, 1024 * 2048), (1, 1024 * 2048 + 1), (3, 1000003)]
OCC_MASKS = ["sparse", "all_off", "all_on", "one_quarter", "under_one", "over_one", "reg_outside", "no_res"]
OCC_LOGITS = ["normal", "diffs", "offset"]
OCC_RESID = ["normal", "edges"]
DIFFS = [0.0, 10.0, -10.0, 20.0, -20.0, 50.0, -50.0, 90.0, -90.0, 200.0, -200.0]
PROB_SHAPES = [(1, 1), (3, 257), (2, 65541)]


def occ_cases(shapes=None, large=True):
    out = [dict(B=B, n=n, mask=m, logits=l, resid=r) for (B, n) in (OCC_SMALL if shapes is None else shapes) for m in OCC_MASKS for l in OCC_LOGITS
           for r in OCC_RESID]
    if large and shapes is None:
        out += [dict(B=B, n=n, mask="sparse", logits="normal", resid="normal") for (B, n) in OCC_LARGE]
    return out


def case_name(c):
    return "-".join(str(v) for v in c.values())


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def make_logits(B, n, regime, rng):
    if regime == "normal":
        return rng.standard_normal((B, 2, n)).astype(np.float32)
    z = np.empty((B, 2, n), dtype=np.float32)
    if regime == "diffs":   # z1 - z0 exactly one of DIFFS, cycling over the cells
        z[:, 0] = np.round(rng.standard_normal((B, n)) * 4) / 4
        k = (np.arange(B * n).reshape(B, n) + int(rng.integers(0, len(DIFFS)))) % len(DIFFS)
        z[:, 1] = z[:, 0] + np.array(DIFFS, dtype=np.float32)[k]
    else:                   # both logits near 1e4, a small difference
        z[:, 0] = 1e4 + 0.5 * rng.standard_normal((B, n))
        z[:, 1] = z[:, 0] + (0.01 * rng.standard_normal((B, n))).astype(np.float32)
    return z


def make_occ(c, poison=True):
    """inputs of one occupancy-loss case; poison: what a mask excludes holds NaN (pos: 255), else zeros (pos: 1)"""
    B, n = c["B"], c["n"]
    rng = np.random.default_rng(_seed("occ", *c.values()))
    beta = np.float32(BETA)
    logit = make_logits(B, n, c["logits"], rng)
    pos = (rng.random((B, n)) < (0.5 if c["logits"] != "normal" else 0.1)).astype(np.uint8)
    mask = c["mask"]
    cm, rm = [(rng.random((B, n)) < q).astype(np.uint8) for q in (0.4, 0.1)]
    cw, rw = rng.random((B, n)).astype(np.float32), rng.random((B, n)).astype(np.float32)
    if mask == "all_off":
        cm[:], rm[:] = 0, 0
    elif mask == "all_on":
        cm[:], rm[:] = 1, 1
    elif mask in ("one_quarter", "under_one", "over_one"):
        cm[:], rm[:] = 0, 0
        k = 1 if mask == "one_quarter" else min(B * n, 3)
        cells = rng.choice(B * n, k, replace=False)
        tot = 0.25 if mask == "one_quarter" else (1.0 - 2.0 ** -20 if mask == "under_one" else 1.0 + 2.0 ** -20)
        for m_, w_ in ((cm, cw), (rm, rw)):
            m_.reshape(-1)[cells] = 1
            w_.reshape(-1)[cells] = np.float32(tot / k)
    elif mask == "reg_outside":
        rm = ((1 - cm) * (rng.random((B, n)) < 0.5)).astype(np.uint8)       # reg_mask only where cls_mask is off
    res = tgt = None
    if mask != "no_res":
        if c["resid"] == "normal":
            res, tgt = rng.standard_normal((B, 3, n)).astype(np.float32), rng.standard_normal((B, 3, n)).astype(np.float32)
        else:   # tgt = 0: d = res exactly; 0, +-beta, one ulp either side, +-1e3, cycling over cells and components
            up, dn = np.nextafter(beta, np.float32(np.inf)), np.nextafter(beta, np.float32(-np.inf))
            edges = np.array([0.0, beta, -beta, up, -up, dn, -dn, 1e3, -1e3], dtype=np.float32)
            k = (np.arange(B * 3 * n).reshape(B, 3, n) + int(rng.integers(0, 9))) % 9
            res, tgt = edges[k], np.zeros((B, 3, n), dtype=np.float32)
    else:
        rm[:] = 0
    bad = np.float32(np.nan) if poison else np.float32(0)
    off_c, off_r = cm == 0, rm == 0
    logit[np.broadcast_to(off_c[:, None], logit.shape)] = bad
    cw[off_c] = bad
    pos[off_c] = 255 if poison else 1
    rw[off_r] = bad
    if res is not None:
        res, tgt = res.copy(), tgt.copy()
        res[np.broadcast_to(off_r[:, None], res.shape)] = bad
        tgt[np.broadcast_to(off_r[:, None], tgt.shape)] = bad
    return dict(logit=logit, res=res, tgt=tgt, pos=pos, cm=cm, cw=cw, rm=rm, rw=rw, beta=BETA, w_cls=W_CLS, w_res=W_RES)


def make_prob(B, n, regime):
    rng = np.random.default_rng(_seed("prob", B, n, regime))
    return make_logits(B, n, regime, rng), (rng.random((B, n)) < 0.5).astype(np.uint8)


SUMSQ_BIG = 1024 * 4096 + 3
SUMSQ_SIZES = [(0, 0), (1, 0), (0, 1), (3, 4), (4, 3), (5, 8), (8, 5), (7, 9), (9, 7), (4095, 4097), (4097, 4095), (4096, 4096), (4096, 1),
               (SUMSQ_BIG, 9), (9, SUMSQ_BIG)]
SUMSQ_TYPES = [("fp32", "fp32"), ("fp32", "bf16"), ("bf16", "fp32"), ("bf16", "bf16"), ("fp32", None), ("bf16", None)]
SUMSQ_ALIGN = [(0, 0), (1, 0), (0, 1), (1, 1)]     # element offset of a, b from a 16-byte aligned base


def sumsq_cases():
    return [dict(na=na, nb=(nb if tb else 0), ta=ta, tb=tb) for (na, nb) in SUMSQ_SIZES for (ta, tb) in SUMSQ_TYPES if tb or nb in (0, 9)]


def make_sumsq(c):
    """-> a, b (float32 values, bf16-representable where the tensor is bf16; b None when absent), ka, kb"""
    rng = np.random.default_rng(_seed("sumsq", *c.values()))
    a = rng.standard_normal(c["na"]).astype(np.float32)
    a = bf16_round(a) if c["ta"] == "bf16" else a
    b = None
    if c["tb"]:
        b = rng.standard_normal(c["nb"]).astype(np.float32)
        b = bf16_round(b) if c["tb"] == "bf16" else b
    return a, b, 1e-3 / max(c["na"], 1), (1e-3 / max(c["nb"], 1) if c["tb"] else 0.0)


ADAM_SMALL = [[1], [1023], [1024], [1025]]
ADAM_LARGE = [[1] * 257, [1] * 513, [7] * 448, [7] * 449, [7] * 897, [5, 1024, 1025, 1, 3000, 2048] + [7] * 460, [300001, 3]]
ADAM_CLIPS = ["off", "huge", "biting", "tiny"]


def adam_regimes():
    return [dict(step=s, wd=wd, beta1=b1, moments=mo) for s in (1, 2, 1000, 10 ** 6) for wd in (0.0, 0.01) for b1 in (0.85, 0.95)
            for mo in ("zero", "random")]


def adam_cases():
    out = [dict(sizes=sz, clip=cl, zero_grad=False, **r) for sz in ADAM_SMALL for cl in ADAM_CLIPS for r in adam_regimes()]
    out += [dict(sizes=sz, clip=cl, zero_grad=True, step=3, wd=0.01, beta1=0.95, moments="zero") for sz in ADAM_SMALL + [[7] * 449] for cl in ("off", "biting")]
    out += [dict(sizes=sz, clip=cl, zero_grad=False, step=3, wd=0.01, beta1=0.95, moments="random") for sz in ADAM_LARGE for cl in ("biting", "off")]
    return out


def adam_name(c):
    sz = c["sizes"]
    s = "x".join(str(v) for v in sz) if len(sz) <= 2 else f"{len(sz)}params{sum(sz)}"
    return "-".join([s] + [str(v) for k, v in c.items() if k != "sizes"])


def make_adam(c):
    """-> grads (list of float32 arrays), p0, m0, v0 (flat float32), hp.  Parameters span six decades so that an error of the size
    of the update shows against a small parameter; biting: norm = 37 clip; tiny: norm 1e-3, clip 1e-4"""
    sizes = c["sizes"]
    nt = sum(sizes)
    rng = np.random.default_rng(_seed("adam", c["clip"], c["zero_grad"], c["step"], c["wd"], c["beta1"], c["moments"], len(sizes), nt))
    g = (rng.standard_normal(nt) * 0.3).astype(np.float32)
    if c["zero_grad"]:
        g[:] = 0
    norm = float(np.sqrt((wide(g) ** 2).sum()))
    clip = 0.0
    if c["clip"] == "huge":
        clip = 1e9
    elif c["clip"] == "biting":
        clip = max(norm, 1.0) / 37.0
    elif c["clip"] == "tiny":
        g = (g * np.float32(1e-3 / max(norm, 1e-30))).astype(np.float32)
        clip = 1e-4
    p0 = (rng.standard_normal(nt) * 10.0 ** rng.uniform(-6, 0, nt)).astype(np.float32)
    if c["moments"] == "zero":
        m0, v0 = np.zeros(nt, np.float32), np.zeros(nt, np.float32)
    else:
        m0, v0 = (rng.standard_normal(nt) * 0.01).astype(np.float32), (rng.random(nt) * 0.01).astype(np.float32)
    grads = list(np.split(g, np.cumsum(sizes)[:-1]))
    hp = dict(step=c["step"], lr=0.003, beta1=c["beta1"], beta2=0.99, eps=1e-8, wd=c["wd"], clip=float(np.float32(clip)))
    return grads, p0, m0, v0, hp


# ------------------------------------------------------------------------------------------------------------------ the checks
class Worst:
    """worst ratio per stage over everything checked through it; strict: a ratio above 1 raises"""

    def __init__(self, strict=True):
        self.worst, self.strict = {}, strict

    def check(self, stage, got, ref_bound, where=""):
        assert stage in STAGES and stage not in EXACT, stage
        return self._note(stage, ratio(got, *ref_bound), where)

    def exact(self, stage, got, ref, where=""):
        """bit-exact stages: ratio 0 or inf"""
        assert stage in EXACT, stage
        got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
        same = got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got.view(np.uint8), ref.view(np.uint8))
        return self._note(stage, 0.0 if same else np.inf, where)

    def _note(self, stage, r, where):
        self.worst[stage] = max(self.worst.get(stage, 0.0), r)
        if self.strict:
            assert r <= 1.0, f"{stage} {where}: |got - ref| is {r:.3g} of its bound"
        return r

    def require(self, cond, where=""):
        """an exact property (zeros outside a mask, untouched moments): asserted when strict, else an infinite ratio under 'exact'"""
        if self.strict:
            assert cond, where
        elif not cond:
            self.worst["exact"] = np.inf

    def report(self):
        return "worst |got - ref| / bound: " + "  ".join(f"{s} {self.worst[s]:.3f}" for s in STAGES if s in self.worst)


def check_occ(W, d, got, where=""):
    """got: S (4 doubles, the sum of the kernel's per-block partials), out (3), norms (2), d_logit, d_res (None without a head),
    g (the upstream gradient pair the backward ran with)"""
    W.check("S", got["S"], occ_sums(d), where)
    o, nm = occ_out(d, got["S"])
    W.check("out", got["out"][:2], o, where)
    W.check("norms", got["norms"], nm, where)
    W.exact("out_total", np.float32(got["out"][2]), np.float32(got["out"][0]) + np.float32(got["out"][1]), where)
    dl, dr = occ_bwd(d, got["norms"], got["g"])
    W.check("d_logit", got["d_logit"], dl, where)
    if d["res"] is not None:
        W.check("d_res", got["d_res"], dr, where)
    else:
        W.require(got["d_res"] is None and float(got["out"][1]) == 0.0, where)
    if not d["cm"].any() and not d["rm"].any():       # all off: exact zeros and norms = w / 1
        W.require(float(got["out"][0]) == 0.0 and float(got["out"][1]) == 0.0 and float(got["out"][2]) == 0.0, where)
        W.require(np.array_equal(np.asarray(got["norms"], np.float32), np.array([d["w_cls"], d["w_res"]], np.float32)), where)
    W.require(not np.any(got["d_logit"][np.broadcast_to(d["cm"][:, None] == 0, got["d_logit"].shape)]), f"{where}: d_logit outside cls_mask")
    if d["res"] is not None:
        W.require(not np.any(got["d_res"][np.broadcast_to(d["rm"][:, None] == 0, got["d_res"].shape)]), f"{where}: d_res outside reg_mask")
    W.require(np.isfinite(got["out"]).all() and np.isfinite(got["norms"]).all(), where)


def check_sumsq(W, a, ka, b, kb, c, got, where=""):
    """got: out (1), da, db (float32 values; db None when b is absent), g"""
    W.check("sumsq2_fwd", got["out"], sumsq2_fwd(a, ka, b, kb), where)
    W.exact("sumsq2_bwd", got["da"], sumsq2_bwd(a, c["ta"] == "bf16", got["g"], np.float32(2.0 * ka)), where)
    if b is not None:
        W.exact("sumsq2_bwd", got["db"], sumsq2_bwd(b, c["tb"] == "bf16", got["g"], np.float32(2.0 * kb)), where)


def check_adam(W, grads, p0, m0, v0, hp, got, where=""):
    """got: tsq (the kernel's total_sq; absent with the clip off), p, m, v, packed"""
    gflat = np.concatenate(grads) if grads else np.zeros(0, np.float32)
    W.exact("grads_pack", got["packed"], gflat, where)
    tsq = 0.0
    if hp["clip"] > 0:
        W.check("total_sq", np.array([got["tsq"]]), total_sq(gflat), where)
        tsq = got["tsq"]
    ref = adam(gflat, p0, m0, v0, tsq, hp)
    for k in ("p", "m", "v"):
        W.check("adam_" + k, got[k], ref[k], where)
    if not np.any(gflat) and not np.any(m0) and not np.any(v0):     # 0 / (0 + eps): the moments stay 0, p is the decayed p exactly
        decay = np.float32(1.0) - np.float32(hp["wd"]) * np.float32(hp["lr"])
        W.require(not np.any(got["m"]) and not np.any(got["v"]) and np.array_equal(got["p"], p0 * decay), where)
