"""tests/bn_ref.py without a GPU: its staged float64 formulas against torch's float64 BatchNorm1d (forward and autograd), and a numpy
emulation of the rounding chain of csrc/bn.hip against its error bounds -- the GPU tests (tests/test_hip_bn_edges.py) inherit bounds
that arithmetic of the kernels' kind demonstrably meets."""
import numpy as np
import pytest
import torch

import bn_ref as R

EPS, MOM = 1e-3, 0.01
F = np.float32


def _close(got, ref, what):
    ref = np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * scale + 1e-300, err_msg=what)


@pytest.mark.parametrize("n,c", [(2, 3), (37, 5), (130, 12)])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("affine", [True, False])
def test_staged_formulas_are_torch_batchnorm_in_float64(n, c, training, relu, affine):
    """each stage fed with the reference's own float64 results of the earlier stages is torch.nn.BatchNorm1d(...).double()"""
    d = R.make_inputs(n, c, 1000 + n + c)
    eps, mom = float(R.f32(EPS)), float(R.f32(MOM))
    bn = torch.nn.BatchNorm1d(c, eps=eps, momentum=mom, affine=affine).double()
    with torch.no_grad():
        bn.running_mean.copy_(torch.from_numpy(d["running_mean"]).double())
        bn.running_var.copy_(torch.from_numpy(d["running_var"]).double())
        if affine:
            bn.weight.copy_(torch.from_numpy(d["gamma"]).double())
            bn.bias.copy_(torch.from_numpy(d["beta"]).double())
    bn.train(training)
    xt = torch.from_numpy(d["x"]).double().requires_grad_(True)
    yt = bn(xt)
    if relu:
        yt = torch.relu(yt)
    yt.backward(torch.from_numpy(d["dy"]).double())

    gamma, beta = (d["gamma"], d["beta"]) if affine else (None, None)
    if training:
        mean, _, rstd = R.stats(d["x"], EPS)
        (rm, _), (rv, _) = R.running(d["x"], d["running_mean"], d["running_var"], MOM, EPS)
        _close(R.mean(d["x"])[0], mean, "mean")
        _close(R.rstd(d["x"], EPS)[0], rstd, "rstd")
    else:
        mean, rstd = R.wide(d["running_mean"]), R.rstd_eval(d["running_var"], EPS)[0]
        rm, rv = R.wide(d["running_mean"]), R.wide(d["running_var"])
    _close(bn.running_mean.numpy(), rm, "running_mean")
    _close(bn.running_var.numpy(), rv, "running_var")
    assert int(bn.num_batches_tracked) == int(training)
    y = R.y(d["x"], mean, rstd, gamma, beta, relu)[0]
    _close(yt.detach().numpy(), y, "y")
    gp = R.masked(d["dy"], yt.detach().numpy(), relu)      # torch's own mask: a constant column without affine sits at y = 0 +- rounding
    db, dg = R.dbeta(gp)[0], R.dgamma(gp, d["x"], mean, rstd)[0]
    if affine:
        _close(bn.bias.grad.numpy(), db, "dbeta")
        _close(bn.weight.grad.numpy(), dg, "dgamma")
    dx = R.dx_train(gp, d["x"], mean, rstd, gamma, dg, db)[0] if training else R.dx_eval(gp, rstd, gamma)[0]
    _close(xt.grad.numpy(), dx, "dx")
    _close(R.col_sum(d["x"])[0], torch.from_numpy(d["x"]).double().sum(0).numpy(), "col_sum")


def test_single_row_training_follows_the_kernels_rule():
    """N = 1 (torch refuses it): variance 0, and the unbiased factor N / (N - 1) is taken as 1"""
    d = R.make_inputs(1, 5, 3)
    mean, var, rstd = R.stats(d["x"], EPS)
    np.testing.assert_array_equal(mean, d["x"][0].astype(np.float64))
    np.testing.assert_array_equal(var, 0.0)
    np.testing.assert_array_equal(rstd, 1.0 / np.sqrt(R.f32(EPS)))
    (rm, _), (rv, _) = R.running(d["x"], d["running_mean"], d["running_var"], MOM, EPS)
    _close(rv, (1.0 - R.f32(MOM)) * d["running_var"].astype(np.float64), "running_var")
    _close(rm, (1.0 - R.f32(MOM)) * d["running_mean"].astype(np.float64) + R.f32(MOM) * mean, "running_mean")


def test_bf16_round_is_torch_bfloat16():
    a = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 37.0
    a[:4] = [0.75, 0.0, 1.00390625, 1.01171875]          # exact, zero, and the two kinds of tie
    np.testing.assert_array_equal(R.bf16_round(a), torch.from_numpy(a).to(torch.bfloat16).float().numpy())


def test_rstd_conditioning_is_asserted():
    x = np.full((4, 1), 4096.0, dtype=np.float32)
    with pytest.raises(AssertionError):
        R.stats(x, 1e-9)


# ---- the kernels' arithmetic in numpy: float32 array operations round every operation on its own (no fma), float64 sums are rounded once
def _emulate(d, training, relu, affine, bf16):
    x, dy = d["x"], d["dy"]
    n, c = x.shape
    g32 = d["gamma"] if affine else np.ones(c, F)
    b32 = d["beta"] if affine else np.zeros(c, F)
    eps, mom = F(EPS), F(MOM)
    out = {}
    if training:                                              # bn_stats: fp64 sums, the last workgroup publishes
        xd = x.astype(np.float64)
        mean = xd.sum(0) / n
        var = np.maximum((xd * xd).sum(0) / n - mean * mean, 0.0)
        out["mean"], out["rstd"] = mean.astype(F), (1.0 / np.sqrt(var + np.float64(eps))).astype(F)
        unb = var * (np.float64(n) / np.float64(n - 1)) if n > 1 else var
        out["running_mean"] = ((1.0 - np.float64(mom)) * d["running_mean"].astype(np.float64) + np.float64(mom) * mean).astype(F)
        out["running_var"] = ((1.0 - np.float64(mom)) * d["running_var"].astype(np.float64) + np.float64(mom) * unb).astype(F)
    else:                                                     # bn_eval_stats
        out["mean"] = d["running_mean"].copy()
        out["rstd"] = (F(1.0) / np.sqrt(d["running_var"] + eps)).astype(F)
    m, rs = out["mean"], out["rstd"]
    t = (((x - m) * rs) * g32) + b32                          # bn_affine
    y = np.maximum(t, F(0)) if relu else t
    out["y"] = R.bf16_round(y) if bf16 else y
    g = np.where(out["y"] > 0, dy, F(0)) if relu else dy      # bn_bwd_stats
    xh = (x - m) * rs
    out["dbeta"] = g.astype(np.float64).sum(0).astype(F)
    out["dgamma"] = (g.astype(np.float64) * xh.astype(np.float64)).sum(0).astype(F)
    s = g32 * rs                                              # bn_bwd_apply
    if training:
        invn = F(1.0) / F(n)
        dx = s * ((g - out["dbeta"] * invn) - (xh * out["dgamma"]) * invn)
    else:
        dx = s * g
    out["dx"] = R.bf16_round(dx) if bf16 else dx
    out["col_sum"] = x.astype(np.float64).sum(0).astype(F)
    assert all(v.dtype == F for v in out.values())
    return out


EMU_SHAPES = [(1, 5), (3, 4), (37, 5), (513, 12), (1000, 34), (262145, 5)]


def test_emulated_kernel_arithmetic_meets_every_bound(capsys):
    """fp32 apply, fp64 sums rounded once, bn_bwd_apply in fp32 (and bf16 storage of y / dx): every stage within its bound, worst
    ratio per stage printed (the figures in bn_ref's docstring)"""
    W = R.Worst()
    for bf16 in (False, True):
        for i, (n, c) in enumerate(EMU_SHAPES):
            d = R.make_inputs(n, c, 7 * i + 1, bf16)
            for training, relu, affine in ((True, True, True), (True, False, False), (False, True, True), (False, False, True)):
                got = _emulate(d, training, relu, affine, bf16)
                R.check_all(W, "bf16" if bf16 else "fp32", d, got, training, relu, affine, bf16, MOM, EPS,
                            f"N={n} C={c} training={training} relu={relu} affine={affine}")
    assert {s for s, _ in W.worst} == set(R.STAGES)
    with capsys.disabled():
        print("\n" + W.report())


def test_a_wrong_stage_is_caught():
    """the bounds are tight enough to see ONE chain of fp32 additions over all rows, and a dropped row"""
    d = R.make_inputs(4097, 5, 11)
    got = _emulate(d, True, True, True, False)
    gp = R.masked(d["dy"], got["y"], True)
    acc = F(0) * got["dbeta"]
    for row in np.where(got["y"] > 0, d["dy"], F(0)):        # dbeta accumulated in float32
        acc = acc + row
    assert R.ratio(acc, *R.dbeta(gp)) > 1.0
    dropped = d["x"][:-1].astype(np.float64).sum(0).astype(F)  # col_sum without its last row
    assert R.ratio(dropped, *R.col_sum(d["x"])) > 1.0
    with pytest.raises(AssertionError, match="mean"):
        R.Worst().check("mean", "fp32", d["x"][:-1].astype(np.float64).mean(0).astype(F), R.mean(d["x"]), "without the last row")
