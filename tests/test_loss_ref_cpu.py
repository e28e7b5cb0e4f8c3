"""tests/loss_ref.py without a GPU: its formulas against independent float64 implementations (torch autograd of the formulation in
test_hip_abi_contract._occ_loss_ref, oracle.occ_oracle.occ_losses, clip_grad_norm_ + decoupled decay + torch.optim.Adam, the torch
one-liners of sumsq2 and occ_prob) at 1e-12 relative; a numpy fp32 emulation of every kernel -- each operation rounded to float32 on
its own, the kernels' grids, grid strides, summation orders, chunk tables and launch loops -- against the bounds, over the case
lists tests/test_hip_loss_optim_edges.py runs on the GPU; and thirteen seeded defects of that emulation, each of which must push
some case of those lists over its bound in the stage it belongs to (so that the GPU module cannot pass vacuously)."""
import numpy as np
import pytest
import torch

import loss_ref as R
from bn_ref import bf16_round, wide

F1 = np.float32(1.0)
DEFECTS = {   # defect -> the stage in which a case of the shared lists must exceed its bound
    "no_eps": "S", "no_clamp": "out", "skip_second_iteration": "S", "drop_partials_from_64": "S", "beta_wrong_side": "S", "swap_d_logit": "d_logit",
    "stale_pointer_table": "adam_p", "total_stops_at_256": "total_sq", "inv_bc2": "adam_p", "decay_after_update": "adam_p",
    "no_clip_eps": "adam_p", "extra_vector": "sumsq2_fwd", "swap_bf16_halves": "sumsq2_bwd",
}


def cdiv(a, b):
    return -(-a // b)


def wave_tree(a, first=32):
    """__shfl_down tree over the last axis (64 lanes), offsets first .. 1 -> lane 0"""
    a = a.copy()
    o = first
    while o >= 1:
        a[..., :o] += a[..., o:2 * o]
        o //= 2
    return a[..., 0]


def strided_accumulate(terms, threads):
    """terms (..., n) in element order; thread t adds elements t, t + threads, ... in order -> (..., threads), float64"""
    n = terms.shape[-1]
    it = max(cdiv(n, threads), 1)
    pad = np.zeros(terms.shape[:-1] + (it * threads,), dtype=np.float64)
    pad[..., :n] = terms
    pad = pad.reshape(terms.shape[:-1] + (it, threads))
    acc = np.zeros(terms.shape[:-1] + (threads,), dtype=np.float64)
    for k in range(it):
        acc = acc + pad[..., k, :]
    return acc, pad


# ------------------------------------------------------------------------------------------------------------------ emulations
def emu_softmax(z0, z1):
    m = np.maximum(z0, z1)
    e0, e1 = np.exp(z0 - m), np.exp(z1 - m)
    return e0, e1, F1 / (e0 + e1)


def emu_occ(d, g, defect=None):
    """occ_loss_fwd + occ_loss_bwd of csrc/occ_loss.hip in numpy float32 -> the dict loss_ref.check_occ takes"""
    B, _, n = d["logit"].shape
    total = B * n
    beta, eps = np.float32(d["beta"]), np.float32(1e-6)
    cm, rm = d["cm"].reshape(-1) != 0, d["rm"].reshape(-1) != 0
    pos = d["pos"].reshape(-1) != 0
    z0, z1 = d["logit"][:, 0].reshape(-1), d["logit"][:, 1].reshape(-1)
    cw, rw = d["cw"].reshape(-1), d["rw"].reshape(-1)
    with np.errstate(all="ignore"):
        e0, e1, inv = emu_softmax(z0, z1)
        s0, s1 = e0 * inv, e1 * inv
        st, so = np.where(pos, s1, s0), np.where(pos, s0, s1)
        p = st if defect == "no_eps" else st + eps
        om = F1 - p
        fl = -(om * om) * np.log(p)
        terms = np.zeros((4, total))
        terms[0] = np.where(cm, wide(cw) * wide(fl), 0.0)
        terms[1] = np.where(cm, wide(cw), 0.0)
        if d["res"] is not None:
            sl = []
            for k in range(3):
                ad = np.abs(d["res"][:, k].reshape(-1) - d["tgt"][:, k].reshape(-1))
                quad = np.float32(0.5) * ad * ad if defect == "beta_wrong_side" else np.float32(0.5) * ad * ad / beta
                sl.append(np.where(ad < beta, quad, ad - np.float32(0.5) * beta))
            terms[2] = np.where(rm, wide(rw) * ((wide(sl[0]) + wide(sl[1])) + wide(sl[2])), 0.0)
            terms[3] = np.where(rm, wide(rw), 0.0)
    grid = min(max(cdiv(total, 2048), 1), 1024)
    acc, pad = strided_accumulate(terms, grid * 256)
    if defect == "skip_second_iteration" and pad.shape[1] > 1:
        acc = acc - pad[:, 1, :]
    w = wave_tree(acc.reshape(4, grid, 4, 64))                        # (4, grid, 4 waves)
    partial = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]       # (4, grid)
    if defect == "drop_partials_from_64":
        partial = partial[:, :64]
    v, _ = strided_accumulate(partial, 64)                            # thread (j, q): blocks j, j + 64, ...
    v = v.reshape(4, 4, 16)                                           # a wave holds 16 consecutive j of each quantity
    o = 8
    while o >= 1:
        v[..., :o] += v[..., o:2 * o]
        o //= 2
    v = v[..., 0]
    S = (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])
    nc, nr = (S[1], S[3]) if defect == "no_clamp" else (max(S[1], 1.0), max(S[3], 1.0))
    nc, nr = (nc or 1.0), (nr or 1.0)
    w_cls, w_res = float(np.float32(d["w_cls"])), float(np.float32(d["w_res"]))
    out = np.zeros(3, np.float32)
    out[0], out[1] = np.float32(S[0] / nc * w_cls), np.float32(S[2] / nr * w_res)
    out[2] = out[0] + out[1]
    norms = np.array([w_cls / nc, w_res / nr]).astype(np.float32)
    # backward
    g = np.asarray(g, np.float32)
    with np.errstate(all="ignore"):
        dfdp = np.float32(2.0) * om * np.log(p) - om * om / p
        scale = g[0] * norms[0] * cw * dfdp
        dt, do = scale * st * (F1 - st), -scale * st * so
        d0, d1 = np.where(pos, do, dt), np.where(pos, dt, do)
        if defect == "swap_d_logit":
            d0, d1 = np.where(pos, d1, d0), np.where(pos, d0, d1)
        dl = np.stack([np.where(cm, d0, F1 * 0).reshape(B, n), np.where(cm, d1, F1 * 0).reshape(B, n)], 1).astype(np.float32)
        dr = None
        if d["res"] is not None:
            sc = g[1] * norms[1] * rw
            dr = np.zeros((B, 3, n), np.float32)
            for k in range(3):
                dd = d["res"][:, k].reshape(-1) - d["tgt"][:, k].reshape(-1)
                gr = np.where(np.abs(dd) < beta, dd / beta, np.sign(dd).astype(np.float32))
                dr[:, k] = np.where(rm, sc * gr, F1 * 0).reshape(B, n)
    return dict(S=S, out=out, norms=norms, d_logit=dl, d_res=dr, g=g)


def emu_occ_prob(logit, mask):
    e0, e1, _ = emu_softmax(logit[:, 0], logit[:, 1])
    return (e1 / (e0 + e1)) * mask.astype(np.float32)


def emu_sumsq_tensor(x, bf, aligned, threads, defect):
    n = x.size
    acc = np.zeros(threads)
    done = 0
    if aligned:
        epv = 8 if bf else 4
        nv = n // epv
        done = nv * epv
        if defect == "extra_vector":
            nv += 1
        xp = np.ones(nv * epv, np.float32)                            # (what lies behind the tensor: ones)
        xp[:min(n, nv * epv)] = x[:nv * epv]
        v = xp.reshape(nv, epv)
        s = np.zeros(nv, np.float32)
        for j in range(4):
            s = s + ((v[:, 2 * j] * v[:, 2 * j] + v[:, 2 * j + 1] * v[:, 2 * j + 1]) if bf else v[:, j] * v[:, j])
        acc = acc + strided_accumulate(wide(s), threads)[0]
    return acc + strided_accumulate(wide(x[done:]) ** 2, threads)[0]


def emu_sumsq(a, ka, b, kb, c, align, g, defect=None):
    na, nb = a.size, (b.size if b is not None else 0)
    grid = min(max(cdiv(max(na, nb, 1), 4096), 1), 1024)
    T = grid * 256
    acc = emu_sumsq_tensor(a, c["ta"] == "bf16", align[0] % (8 if c["ta"] == "bf16" else 4) == 0, T, defect) * ka
    if b is not None:
        acc = acc + emu_sumsq_tensor(b, c["tb"] == "bf16", align[1] % (8 if c["tb"] == "bf16" else 4) == 0, T, defect) * kb
    w = wave_tree(acc.reshape(grid, 4, 64))
    partial = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    w = wave_tree(strided_accumulate(partial, 256)[0].reshape(4, 64))
    out = np.array([(w[0] + w[1]) + (w[2] + w[3])]).astype(np.float32)
    g = np.float32(g)
    da = R.sumsq2_bwd(a, c["ta"] == "bf16", g, np.float32(2.0 * ka))
    if defect == "swap_bf16_halves" and c["ta"] == "bf16":           # the two halves of every 32-bit word of a exchanged (the forward sum is
        h = (na // 2) * 2                                             # symmetric in them: only the backward can show it)
        da = da.copy()
        da[:h] = da[:h].reshape(-1, 2)[:, ::-1].reshape(-1)
    db = R.sumsq2_bwd(b, c["tb"] == "bf16", g, np.float32(2.0 * kb)) if b is not None else None
    return dict(out=out, da=da, db=db, g=g)


def emu_adam(grads, p0, m0, v0, hp, defect=None):
    """btc_grads_pack + btc_adam_group_step of csrc/optim.hip: chunk tables, one pointer table per launch of <= 448 parameters"""
    sizes = [x.size for x in grads]
    t = R.chunk_tables_np(sizes)
    nch, nseg, MS = len(t["seg"]), len(sizes), R.ADAM_MAX_SEGMENTS
    rows = np.zeros((nch, 1024), np.float32)                          # the gradient elements each chunk's workgroup reads
    for s0 in range(0, nseg, MS):
        table = grads[0:MS] if (defect == "stale_pointer_table" and s0) else grads[s0:s0 + MS]
        for c in range(t["seg0"][s0], t["seg0"][min(s0 + MS, nseg)]):
            src = table[t["seg"][c]][t["off"][c]:t["off"][c] + t["len"][c]]
            rows[c, :src.size] = src
    lens = t["len"].astype(np.int64)
    valid = np.arange(1024)[None, :] < lens[:, None]
    packed = np.zeros(sum(sizes), np.float32)
    flat_idx = (t["flat"][:, None] + np.arange(1024)[None, :])[valid]
    packed[flat_idx] = rows[valid]
    out = dict(packed=packed)
    clip = np.float32(hp["clip"])
    inv_coef = F1
    if clip > 0:
        acc, _ = strided_accumulate(wide(rows) ** 2, 256)             # (chunk, 256 threads): elements e, e + 256, ...
        w = wave_tree(acc.reshape(nch, 4, 64))
        partial = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
        if defect == "total_stops_at_256":
            partial = partial[:256]
        tsq = 0.0
        for x in strided_accumulate(partial, 256)[0]:
            tsq += x
        out["tsq"] = tsq
        norm = np.float32(np.sqrt(tsq))
        inv_coef = np.maximum((norm if defect == "no_clip_eps" else norm + np.float32(1e-6)) / clip, F1)
    lr, b1, b2, eps, wd = (np.float32(hp[k]) for k in ("lr", "beta1", "beta2", "eps", "wd"))
    bc1, bc2 = 1.0 - float(b1) ** hp["step"], 1.0 - float(b2) ** hp["step"]
    decay, lob = F1 - wd * lr, np.float32(float(lr) / bc1)
    isb = np.float32(1.0 / bc2) if defect == "inv_bc2" else np.float32(1.0 / np.sqrt(bc2))
    gr = packed / inv_coef
    mv = m0 + (F1 - b1) * (gr - m0)
    vv = b2 * v0 + (F1 - b2) * gr * gr
    denom = np.sqrt(vv) * isb + eps
    if defect == "decay_after_update":
        pv = (p0 - lob * mv / denom) * decay
    else:
        pv = p0 * decay - lob * mv / denom
    out.update(p=pv.astype(np.float32), m=mv.astype(np.float32), v=vv.astype(np.float32))
    return out


# ------------------------------------------------------------------------------------------------------------------ runners
def run_occ(W, cases, defect=None):
    for c in cases:
        d = R.make_occ(c)
        R.check_occ(W, d, emu_occ(d, (R.G_UP, R.G_UP), defect), R.case_name(c))


def run_prob(W):
    for B, n in R.PROB_SHAPES:
        for regime in R.OCC_LOGITS:
            logit, mask = R.make_prob(B, n, regime)
            W.check("occ_prob", emu_occ_prob(logit, mask), R.occ_prob(logit, mask), f"{B}x{n} {regime}")


def run_sumsq(W, cases, defect=None):
    for c in cases:
        a, b, ka, kb = R.make_sumsq(c)
        for al in R.SUMSQ_ALIGN:
            R.check_sumsq(W, a, ka, b, kb, c, emu_sumsq(a, ka, b, kb, c, al, R.G_UP, defect), f"{c} align {al}")


def run_adam(W, cases, defect=None):
    for c in cases:
        grads, p0, m0, v0, hp = R.make_adam(c)
        R.check_adam(W, grads, p0, m0, v0, hp, emu_adam(grads, p0, m0, v0, hp, defect), R.adam_name(c))


SMALL_SUMSQ = [c for c in R.sumsq_cases() if max(c["na"], c["nb"]) < R.SUMSQ_BIG]
WORST = R.Worst()


# ------------------------------------------------------------------------------------------------------------------ formulas
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300)) if a.size else 0.0


PY_EPS = 1e-6     # the independent implementations add the Python float 1e-6, the kernel float32(1e-6): the formula checks align it


@pytest.mark.parametrize("logits", R.OCC_LOGITS)
@pytest.mark.parametrize("mask", ["sparse", "all_on", "one_quarter", "under_one", "over_one", "reg_outside"])
@pytest.mark.parametrize("shape", [(1, 63), (3, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_occ_formulas_match_torch_float64_autograd(shape, mask, logits):
    from test_hip_abi_contract import _occ_loss_ref
    for resid in R.OCC_RESID:
        d = R.make_occ(dict(B=shape[0], n=shape[1], mask=mask, logits=logits, resid=resid), poison=False)
        beta, wc, wr = (float(np.float32(v)) for v in (d["beta"], d["w_cls"], d["w_res"]))
        l, r, cls, reg = _occ_loss_ref(d["logit"], d["res"], d["tgt"], (d["pos"] != 0).astype(np.uint8), d["cm"], d["cw"], d["rm"], d["rw"], beta, wc, wr)
        g = (0.7, 0.3)
        (float(np.float32(g[0])) * cls + float(np.float32(g[1])) * reg).backward()
        S, _ = R.occ_sums(d, PY_EPS)
        (out, _), (norms, _) = R.occ_out(d, S)
        (dl, _), (dr, _) = R.occ_bwd(d, norms, g, PY_EPS)
        cls, reg = float(cls.detach()), float(reg.detach())
        assert abs(out[0] - cls) <= 1e-12 * abs(cls) and abs(out[1] - reg) <= 1e-12 * abs(reg)
        # (relative to the largest element, plus 1e-14: torch's softmax is rounded to 2^-53 ABSOLUTE, so where one class saturates its
        # gradient is 0 and 1 - p carries the cancellation; scale = g norms w dfdp is of order 1 to 10 here)
        tl = l.grad.numpy()
        assert np.abs(dl - tl).max() <= 1e-12 * np.abs(tl).max() + 1e-14 and _rel(dr, r.grad.numpy()) <= 1e-12


def test_occ_formulas_match_the_oracle():
    from oracle import occ_oracle
    d = R.make_occ(dict(B=3, n=257, mask="sparse", logits="normal", resid="normal"), poison=False)
    B, n = d["cm"].shape
    t5 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double().reshape(a.shape[:-1] + (1, 1, n))
    bd = dict(pos_mask=torch.from_numpy(d["pos"] != 0).reshape(B, 1, 1, n), pred_occ_logit=t5(d["logit"]), pred_sem_residuals=t5(d["res"]),
              res_mtrx=t5(d["tgt"]), general_cls_loss_mask=torch.from_numpy(d["cm"] != 0).reshape(B, 1, 1, n),
              general_cls_loss_mask_float=t5(d["cw"]), general_reg_loss_mask=torch.from_numpy(d["rm"] != 0).reshape(B, 1, 1, n),
              general_reg_loss_mask_float=t5(d["rw"]))
    lw = dict(res_beta=float(np.float32(d["beta"])), occ_fore_cls_weight=float(np.float32(d["w_cls"])), occ_fore_res_weight=float(np.float32(d["w_res"])))
    _, cls, reg = occ_oracle.occ_losses(bd, lw)
    S, _ = R.occ_sums(d, PY_EPS)
    (out, _), _ = R.occ_out(d, S)
    assert abs(out[0] - float(cls)) <= 1e-12 * abs(float(cls)) and abs(out[1] - float(reg)) <= 1e-12 * abs(float(reg))


@pytest.mark.parametrize("clip", R.ADAM_CLIPS)
def test_adam_formulas_match_torch_float64(clip):
    """clip_grad_norm_, p *= 1 - wd lr, torch.optim.Adam in float64, five steps with fresh gradients"""
    c = dict(sizes=[5, 1025, 3], clip=clip, zero_grad=False, step=1, wd=0.01, beta1=0.95, moments="zero")
    grads, p0, m0, v0, hp = R.make_adam(c)
    lr, b1, b2, eps, wd = (float(np.float32(hp[k])) for k in ("lr", "beta1", "beta2", "eps", "wd"))
    params = [torch.nn.Parameter(torch.from_numpy(x).double()) for x in np.split(p0, np.cumsum(c["sizes"])[:-1])]
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=0.0)
    p, m, v = p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    rng = np.random.default_rng(5)
    for step in range(1, 6):
        gs = [(x * rng.uniform(0.5, 2.0)).astype(np.float32) for x in grads]
        for q, x in zip(params, gs):
            q.grad = torch.from_numpy(x).double()
        if hp["clip"] > 0:
            torch.nn.utils.clip_grad_norm_(params, float(np.float32(hp["clip"])))
        with torch.no_grad():
            for q in params:
                q.mul_(1.0 - wd * lr)
        opt.step()
        gflat = np.concatenate(gs)
        ref = R.adam(gflat, p, m, v, R.total_sq(gflat)[0][0], dict(hp, step=step, clip_eps=PY_EPS))
        p, m, v = ref["p"][0], ref["m"][0], ref["v"][0]
        tp = np.concatenate([q.detach().numpy() for q in params])
        tm = np.concatenate([opt.state[q]["exp_avg"].numpy() for q in params])
        tv = np.concatenate([opt.state[q]["exp_avg_sq"].numpy() for q in params])
        assert _rel(p, tp) <= 1e-12 and _rel(m, tm) <= 1e-12 and _rel(v, tv) <= 1e-12, step


def test_sumsq2_and_occ_prob_match_their_torch_one_liners():
    for c in SMALL_SUMSQ:
        a, b, ka, kb = R.make_sumsq(c)
        ta = torch.from_numpy(a).double()
        ref = ka * (ta ** 2).sum() + (kb * (torch.from_numpy(b).double() ** 2).sum() if b is not None else 0.0)
        assert abs(R.sumsq2_fwd(a, ka, b, kb)[0][0] - float(ref)) <= 1e-12 * abs(float(ref))
        for x, k, bf in ((a, ka, c["ta"] == "bf16"), (b, kb, c["tb"] == "bf16")):
            if x is None:
                continue
            t = torch.from_numpy(x).to(torch.bfloat16 if bf else torch.float32)
            g = torch.tensor(R.G_UP, dtype=torch.float32)
            want = (t * (g * float(np.float32(2.0 * k))).to(t.dtype)).float().numpy()      # MeanSquare2.backward's torch branch
            assert np.array_equal(R.sumsq2_bwd(x, bf, R.G_UP, np.float32(2.0 * k)), want)
    for B, n in R.PROB_SHAPES:
        for regime in R.OCC_LOGITS:
            logit, mask = R.make_prob(B, n, regime)
            ref = torch.softmax(torch.from_numpy(logit).double(), dim=1)[:, 1] * torch.from_numpy(mask).double()
            assert np.abs(R.occ_prob(logit, mask)[0] - ref.numpy()).max() <= 1e-12


def test_chunk_tables_twin_wraps_the_pointer_table():
    t = R.chunk_tables_np([7] * 449 + [2049])
    assert t["seg"][448] == 0 and t["seg"][449] == 1 and t["seg0"][-1] == 452 and list(t["off"][449:]) == [0, 1024, 2048]
    assert list(t["len"][449:]) == [1024, 1024, 1] and t["flat"][451] == 7 * 449 + 2048


# ------------------------------------------------------------------------------------------------------------------ emulation vs bounds
@pytest.mark.parametrize("shape", R.OCC_SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_emulated_occ_loss_meets_the_bounds(shape):
    run_occ(WORST, R.occ_cases([shape]))


@pytest.mark.parametrize("shape", R.OCC_LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_emulated_occ_loss_meets_the_bounds_at_the_grid_edges(shape):
    run_occ(WORST, [dict(B=shape[0], n=shape[1], mask="sparse", logits="normal", resid="normal")])


def test_emulated_occ_prob_meets_the_bounds():
    run_prob(WORST)


@pytest.mark.parametrize("sizes", R.SUMSQ_SIZES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_emulated_sumsq2_meets_the_bounds(sizes):
    run_sumsq(WORST, [c for c in R.sumsq_cases() if (c["na"], c["nb"]) in (sizes, (sizes[0], 0))])


def test_emulated_adam_meets_the_bounds():
    run_adam(WORST, R.adam_cases())


def test_poison_changes_nothing_in_the_reference():
    c = dict(B=3, n=257, mask="sparse", logits="normal", resid="normal")
    a, b = R.make_occ(c, poison=True), R.make_occ(c, poison=False)
    assert np.array_equal(R.occ_sums(a)[0], R.occ_sums(b)[0])
    assert np.isnan(a["logit"]).any() and np.isnan(a["res"]).any() and np.isnan(a["cw"]).any() and (a["pos"] == 255).any()


# ------------------------------------------------------------------------------------------------------------------ the cases can fail
DEFECT_CASES = {   # where to look (all of them cases of the shared lists)
    "occ": R.occ_cases([(1, 1), (1, 257), (3, 257), (1, 2049)], large=False),
    "occ_large": [dict(B=B, n=n, mask="sparse", logits="normal", resid="normal") for (B, n) in R.OCC_LARGE],
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_a_seeded_defect_exceeds_a_bound(defect):
    W = R.Worst(strict=False)
    stage = DEFECTS[defect]
    with np.errstate(invalid="ignore"):                               # (a defect may well produce inf - inf: an infinite ratio)
        _run_defect(W, stage, defect)
    assert W.worst[stage] > 1.0, f"{defect}: no case exceeds its bound in {stage} (worst {W.worst[stage]:.3g})"


def _run_defect(W, stage, defect):
    if defect in ("skip_second_iteration", "drop_partials_from_64"):
        run_occ(W, [DEFECT_CASES["occ_large"][3 if defect == "skip_second_iteration" else 0]], defect)
    elif stage in ("S", "out", "d_logit"):
        run_occ(W, DEFECT_CASES["occ"], defect)
    elif stage.startswith("sumsq2"):
        run_sumsq(W, SMALL_SUMSQ, defect)
    else:
        run_adam(W, [c for c in R.adam_cases() if c["sizes"] in R.ADAM_LARGE + [[1025]]], defect)


def test_report_worst_emulation_ratios(capsys):
    """last in the file: the figures recorded in the docstring of tests/loss_ref.py"""
    assert all(r <= 1.0 for r in WORST.worst.values())
    with capsys.disabled():
        print("\n" + WORST.report())
