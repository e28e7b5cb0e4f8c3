"""Float64 reference of fused BatchNorm1d(+ReLU) and of the column sum (csrc/bn.hip), stage by stage, with a derived error
bound for every stage.  Plain numpy: no GPU, no autograd.

Every stage is judged on its own: a stage that consumes an earlier result takes the KERNEL's returned value of it (the fp32
mean / rstd for y, the kernel's y for the ReLU mask, the kernel's dgamma / dbeta for dx), widened to float64, so that a correct
dx cannot hide a wrong dgamma and one rounding is not charged twice.  Inputs are widened first (bfloat16 widens exactly);
momentum and eps are float64(float32(v)), because the C ABI takes floats.

Each function returns (reference, bound); `ratio` gives max |got - ref| / bound, and a ratio above 1 is a failure.

  stage          reference                                          bound on |got - ref|  (every bound + 1e-30)
  mean           sum x / N                                          2^-23 |ref| + 2^-40 sum|x| / N
  rstd           1 / sqrt(max(sum x^2 / N - mean^2, 0) + eps)       2^-22 ref
  running mean   (1 - m) old + m mean                               2^-22 |ref|
  running var    (1 - m) old + m var N / (N - 1)   (N = 1: m var)   2^-22 |ref|
  y              t = (x - mean_k) rstd_k g,  y = relu?(t + b)       2^-21 (|t| + |b|)              bf16: + 2^-8 |ref|
  dbeta          sum g',  g' = dy (y_k > 0)                         2^-23 |ref| + 2^-40 sum|g'|
  dgamma         sum g' xh,  xh = (x - mean_k) rstd_k               2^-22 sum|g' xh| + 2^-23 |ref|
  dx, training   g rstd_k (g' - dbeta_k / N - xh dgamma_k / N)      2^-20 |g rstd_k| (|g'| + |dbeta_k| / N + |xh dgamma_k| / N)
                                                                                                   bf16: + 2^-8 |ref|
  dx, eval       g rstd_k g'                                        2^-22 |ref|                    bf16: + 2^-8 |ref|
  col_sum        sum x                                              2^-23 |ref| + 2^-40 sum|x|

Where the bounds come from.  The kernels accumulate every cross-row sum in float64 and round it to fp32 once (2^-24 relative);
the elementwise kernels work in fp32 with every operation rounded on its own: bn_affine has four roundings on t and one shared
with b, 2^-24 (4 |t| + |b|) to first order; the backward statistics round (x - mean) and its product with rstd; bn_bwd_apply has
about eight roundings over its three terms.  Every bound is at least twice that first-order count.  bfloat16 storage adds one
rounding to 8 significant bits: at most 2^-8 of the stored value, so the 2^-8 |ref| term has no slack of its own (the fp32 part of
the bound, which the fp32 arithmetic only half uses, absorbs the difference between the value before rounding and ref).

The variance comes from sum x^2 / N - mean^2 in float64.  Its cancellation error is about 2^-52 sum x^2 / N, i.e. a relative error of
2^-52 K in rstd with K = (sum x^2 / N) / (var + eps).  `stats` asserts K <= 2^24 (RSTD_COND): the cancellation then stays below 2^-28,
a sixteenth of the 2^-24 the rounding to fp32 takes and far inside the 2^-22 bound.  (A single row with |x| = 30 and eps = 1e-3 has
K = 9e5; K <= 2^10 would rule out every shape of a few rows whose mean is far from zero, which are the shapes of interest here.)

The eval-mode rstd is 1 / sqrtf(running_var + eps) in fp32: three correctly rounded operations, at most (1/2 + 1 + 1) 2^-24 < 2^-22.

tests/test_bn_ref_cpu.py ties these formulas to torch's float64 BatchNorm1d (forward and autograd, 1e-12 relative) and runs a numpy
emulation of the kernels' rounding chain against the bounds.  Worst ratio |got - ref| / bound of that emulation per stage
(fp32 | bf16 activations; six shapes from 1 x 5 to 262145 x 5, a constant column and a column with its mean 30 deviations out):

  mean 0.477 | 0.460    rstd 0.396 | 0.396    running_mean 0.236 | 0.236    running_var 0.193 | 0.181    y 0.358 | 0.996
  dbeta 0.489 | 0.389   dgamma 0.259 | 0.209  dx_train 0.278 | 0.996        dx_eval 0.465 | 0.981        col_sum 0.473 | 0.489
"""
import numpy as np

TINY = 1e-30
RSTD_COND = 2.0 ** 24


def f32(v):
    """a Python float as the C ABI receives it"""
    return np.float64(np.float32(v))


def wide(a):
    return np.asarray(a, dtype=np.float64)


def bf16_round(a):
    """nearest bfloat16 (ties to even) of finite float32 values, returned as float32"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound; inf where got is not finite"""
    got, ref, bound = wide(got), wide(ref), wide(bound)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.size == 0:
        return 0.0
    r = np.abs(got - ref) / bound
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max())


def stats(x, eps):
    """-> mean, biased var, rstd of the columns of x (N, C); asserts the conditioning the rstd bound assumes"""
    x = wide(x)
    n = x.shape[0]
    mean = x.sum(0) / n
    ex2 = (x * x).sum(0) / n
    var = np.maximum(ex2 - mean * mean, 0.0)
    assert np.all(ex2 <= RSTD_COND * (var + f32(eps))), "input too ill-conditioned for the rstd bound"
    return mean, var, 1.0 / np.sqrt(var + f32(eps))


def mean(x):
    x = wide(x)
    n = x.shape[0]
    ref = x.sum(0) / n
    return ref, 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * np.abs(x).sum(0) / n + TINY


def rstd(x, eps):
    ref = stats(x, eps)[2]
    return ref, 2.0 ** -22 * ref + TINY


def rstd_eval(running_var, eps):
    ref = 1.0 / np.sqrt(wide(running_var) + f32(eps))
    return ref, 2.0 ** -22 * ref + TINY


def running(x, old_mean, old_var, momentum, eps):
    """-> (running mean, bound), (running var, bound) after one training step"""
    m = f32(momentum)
    mu, var, _ = stats(x, eps)
    n = wide(x).shape[0]
    unb = var * (n / (n - 1.0)) if n > 1 else var
    rm = (1.0 - m) * wide(old_mean) + m * mu
    rv = (1.0 - m) * wide(old_var) + m * unb
    return (rm, 2.0 ** -22 * np.abs(rm) + TINY), (rv, 2.0 ** -22 * np.abs(rv) + TINY)


def _affine(c, gamma, beta):
    g = np.ones(c) if gamma is None else wide(gamma)
    b = np.zeros(c) if beta is None else wide(beta)
    return g, b


def y(x, mean_k, rstd_k, gamma, beta, relu, bf16=False):
    x = wide(x)
    g, b = _affine(x.shape[1], gamma, beta)
    t = (x - wide(mean_k)) * wide(rstd_k) * g
    ref = t + b
    if relu:
        ref = np.maximum(ref, 0.0)
    bound = 2.0 ** -21 * (np.abs(t) + np.abs(b)) + TINY
    if bf16:
        bound = bound + 2.0 ** -8 * np.abs(ref)
    return ref, bound


def masked(dy, y_k, relu):
    """g' = dy where the kernel's own output is positive (all of dy without ReLU)"""
    return wide(dy) * (wide(y_k) > 0) if relu else wide(dy)


def xhat(x, mean_k, rstd_k):
    return (wide(x) - wide(mean_k)) * wide(rstd_k)


def dbeta(gp):
    ref = gp.sum(0)
    return ref, 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * np.abs(gp).sum(0) + TINY


def dgamma(gp, x, mean_k, rstd_k):
    p = gp * xhat(x, mean_k, rstd_k)
    ref = p.sum(0)
    return ref, 2.0 ** -22 * np.abs(p).sum(0) + 2.0 ** -23 * np.abs(ref) + TINY


def dx_train(gp, x, mean_k, rstd_k, gamma, dgamma_k, dbeta_k, bf16=False):
    x = wide(x)
    n = x.shape[0]
    g, _ = _affine(x.shape[1], gamma, None)
    s = g * wide(rstd_k)
    xh = xhat(x, mean_k, rstd_k)
    t1, t2 = wide(dbeta_k) / n, xh * wide(dgamma_k) / n
    ref = s * (gp - t1 - t2)
    bound = 2.0 ** -20 * np.abs(s) * (np.abs(gp) + np.abs(t1) + np.abs(t2)) + TINY
    if bf16:
        bound = bound + 2.0 ** -8 * np.abs(ref)
    return ref, bound


def dx_eval(gp, rstd_k, gamma, bf16=False):
    g, _ = _affine(gp.shape[1], gamma, None)
    ref = g * wide(rstd_k) * gp
    bound = 2.0 ** -22 * np.abs(ref) + TINY
    if bf16:
        bound = bound + 2.0 ** -8 * np.abs(ref)
    return ref, bound


def col_sum(x):
    x = wide(x)
    ref = x.sum(0)
    return ref, 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * np.abs(x).sum(0) + TINY


def make_inputs(n, c, seed, bf16=False):
    """the test inputs, float32 numpy: x = mu + sd randn per column with one column the constant 0.75 (exact variance 0) and one
    column at mu = 30, sd = 1; gamma in U(0.5, 1.5), beta in U(-0.5, 0.5), dy = randn, running statistics to start from.
    Fewer than three columns cannot hold both special columns: the seed then decides which one is present.
    bf16: x and dy are rounded to bfloat16 first (and still returned as float32)."""
    rng = np.random.default_rng(seed)
    mu, sd = rng.uniform(-2.0, 2.0, c), rng.uniform(0.5, 2.0, c)
    if c >= 3:
        const_col, far_col = 1, 2
    elif c == 2:
        const_col, far_col = 1, (0 if seed % 2 else None)
    else:
        const_col, far_col = ((None, None), (0, None), (None, 0))[seed % 3]
    if far_col is not None:
        mu[far_col], sd[far_col] = 30.0, 1.0
    x = (mu + sd * rng.standard_normal((n, c))).astype(np.float32)
    if const_col is not None:
        x[:, const_col] = 0.75
    d = dict(x=x, dy=rng.standard_normal((n, c)).astype(np.float32), gamma=rng.uniform(0.5, 1.5, c).astype(np.float32),
             beta=rng.uniform(-0.5, 0.5, c).astype(np.float32), running_mean=rng.uniform(-0.1, 0.1, c).astype(np.float32),
             running_var=rng.uniform(0.5, 1.5, c).astype(np.float32))
    if bf16:
        d["x"], d["dy"] = bf16_round(d["x"]), bf16_round(d["dy"])
    return d


STAGES = ("mean", "rstd", "running_mean", "running_var", "y", "dbeta", "dgamma", "dx_train", "dx_eval", "col_sum")


class Worst:
    """worst ratio per (stage, activation type) over everything checked through it"""

    def __init__(self):
        self.worst = {}

    def check(self, stage, kind, got, ref_bound, where=""):
        assert stage in STAGES, stage
        r = ratio(got, *ref_bound)
        key = (stage, kind)
        self.worst[key] = max(self.worst.get(key, 0.0), r)
        assert r <= 1.0, f"{stage} ({kind}) {where}: |got - ref| is {r:.3g} of its bound"
        return r

    def report(self):
        kinds = sorted({k for _, k in self.worst})
        lines = []
        for kind in kinds:
            parts = [f"{s} {self.worst[(s, kind)]:.3f}" for s in STAGES if (s, kind) in self.worst]
            lines.append(f"worst |got - ref| / bound, {kind}: " + "  ".join(parts))
        return "\n".join(lines)


def check_all(W, kind, d, got, training, relu, affine, bf16, momentum, eps, where):
    """every stage of one forward + backward (`got`: mean, rstd, y, dbeta, dgamma, dx, col_sum and, in training, the running
    statistics) against bn_ref, through the Worst record W.  """
    x, dy = d["x"], d["dy"]
    gamma, beta = (d["gamma"], d["beta"]) if affine else (None, None)
    if training:
        W.check("mean", kind, got["mean"], mean(x), where)
        W.check("rstd", kind, got["rstd"], rstd(x, eps), where)
        if "running_mean" in got:
            rm, rv = running(x, d["running_mean"], d["running_var"], momentum, eps)
            W.check("running_mean", kind, got["running_mean"], rm, where)
            W.check("running_var", kind, got["running_var"], rv, where)
    else:
        assert np.array_equal(got["mean"], d["running_mean"]), where
        W.check("rstd", kind, got["rstd"], rstd_eval(d["running_var"], eps), where)
    W.check("y", kind, got["y"], y(x, got["mean"], got["rstd"], gamma, beta, relu, bf16), where)
    if relu:
        assert float(np.min(got["y"])) >= 0.0, where
    gp = masked(dy, got["y"], relu)
    W.check("dbeta", kind, got["dbeta"], dbeta(gp), where)
    W.check("dgamma", kind, got["dgamma"], dgamma(gp, x, got["mean"], got["rstd"]), where)
    if training:
        W.check("dx_train", kind, got["dx"], dx_train(gp, x, got["mean"], got["rstd"], gamma, got["dgamma"], got["dbeta"], bf16), where)
    else:
        W.check("dx_eval", kind, got["dx"], dx_eval(gp, got["rstd"], gamma, bf16), where)
    if "col_sum" in got:
        W.check("col_sum", kind, got["col_sum"], col_sum(x), where)
