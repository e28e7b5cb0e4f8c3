"""The kernels that make the training loss and apply the update -- csrc/occ_loss.hip, btc_occ_prob and btc_sumsq2_* of csrc/glue.hip,
csrc/optim.hip -- against the float64 reference and the derived bounds of tests/loss_ref.py, stage by stage, over the case lists
tests/test_loss_ref_cpu.py proves able to fail: grids of 1, 2, 66, exactly 1024 and capped with a ragged second and third grid-stride
iteration; saturated softmaxes, logits with a large common offset, sums of weights around the max(sum w, 1) clamp, empty masks, no
residual head, residuals on the smooth-L1 seam; every dtype instance, alignment and vector / tail split of sumsq2; pointer tables of
one, two and three launches, hundreds of chunks, clip off / idle / biting, steps up to 10^6, all-zero gradients.  Every call goes
through the C ABI (ctypes) on a workspace the test owns, with a garbage tail, twice without re-zeroing (bit-identical results), the
occupancy loss once more on inputs whose excluded entries are zeros instead of NaN; one case per family goes through the Python
entry points and must give the ABI's bits.  The worst ratio |got - ref| / bound per stage is printed by the last test."""
import ctypes

import numpy as np
import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu

W = R.Worst()
c_i32p = ctypes.POINTER(ctypes.c_int32)
CANARY, PAD = 12345.0, 5


def dev():
    return torch.device("cuda:0")


def up(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


def nan_like(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())


def bits_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def dirty_ws(nbytes, head=256):
    """zero head, 0xFF (NaN patterns) behind it"""
    ws = torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device=dev())
    ws[:head] = 0
    return ws


def call(name, *args):
    from btcdet_amd._lib import check, lib
    check(getattr(lib(), name)(*args), name)


def head_zero(ws, name):
    assert int(ws[:256].count_nonzero()) == 0, f"{name}: workspace head not left zeroed"


# ------------------------------------------------------------------------------------------------------------------ occupancy loss
def occ_abi(d, ws):
    """all four entry points -> dict of device tensors (S: the per-block partials summed per quantity, float64)"""
    from btcdet_amd._lib import ptr, stream_ptr
    B, _, n = d["logit"].shape
    t = {k: (up(v) if isinstance(v, np.ndarray) else None) for k, v in d.items() if k in ("logit", "res", "tgt", "pos", "cm", "cw", "rm", "rw")}
    args = (ptr(t["logit"]), ptr(t["res"]), ptr(t["tgt"]), ptr(t["pos"]), ptr(t["cm"]), ptr(t["cw"]), ptr(t["rm"]), ptr(t["rw"]), B, n, d["beta"])
    out2, n2, out3, n3 = nan_like((2,)), nan_like((2,)), nan_like((3,)), nan_like((2,))
    call("btc_occ_loss_fwd", *args, d["w_cls"], d["w_res"], ptr(out2), ptr(n2), ptr(ws), ws.numel(), stream_ptr())
    head_zero(ws, "btc_occ_loss_fwd")
    grid = min(max(-(-B * n // 2048), 1), 1024)
    S2 = ws[256:256 + grid * 32].clone().view(torch.float64).reshape(grid, 4)
    call("btc_occ_loss_fwd_total", *args, d["w_cls"], d["w_res"], ptr(out3), ptr(n3), ptr(ws), ws.numel(), stream_ptr())
    head_zero(ws, "btc_occ_loss_fwd_total")
    S3 = ws[256:256 + grid * 32].clone().view(torch.float64).reshape(grid, 4)
    assert bits_equal(out3[:2], out2) and bits_equal(n3, n2) and bits_equal(S2, S3), "the two forward forms differ"
    g2 = torch.full((2,), R.G_UP, dtype=torch.float32, device=dev())
    has_res = d["res"] is not None
    dl2 = torch.zeros((B, 2, n), dtype=torch.float32, device=dev())          # the two-scalar form: pre-zeroed by the caller
    dr2 = torch.zeros((B, 3, n), dtype=torch.float32, device=dev()) if has_res else None
    call("btc_occ_loss_bwd", *args, ptr(n2), ptr(g2), ptr(dl2), ptr(dr2), stream_ptr())
    dl3, dr3 = nan_like((B, 2, n)), (nan_like((B, 3, n)) if has_res else None)  # the total form writes every cell
    call("btc_occ_loss_bwd_total", *args, ptr(n3), ptr(g2[:1].contiguous()), ptr(dl3), ptr(dr3), stream_ptr())
    assert bits_equal(dl3, dl2) and bits_equal(dr3, dr2), "the two backward forms differ"
    return dict(S=S3, out=out3, norms=n3, d_logit=dl3, d_res=dr3)


def to_host(o):
    h = {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}
    h["S"] = h["S"].sum(0)
    h["g"] = (R.G_UP, R.G_UP)
    return h


def run_occ_case(c):
    from btcdet_amd._lib import lib
    d = R.make_occ(c)
    ws = dirty_ws(lib().btc_occ_loss_ws_bytes())
    first = occ_abi(d, ws)
    again = occ_abi(d, ws)                                    # same workspace, not re-zeroed
    clean = occ_abi(R.make_occ(c, poison=False), ws)          # what the masks exclude: zeros instead of NaN
    for k in first:
        assert bits_equal(first[k], again[k]), f"{k} differs between two identical calls, {R.case_name(c)}"
        assert bits_equal(first[k], clean[k]), f"{k} depends on entries its mask excludes, {R.case_name(c)}"
    R.check_occ(W, d, to_host(first), R.case_name(c))
    return d, first


@pytest.mark.parametrize("mask", R.OCC_MASKS)
@pytest.mark.parametrize("shape", R.OCC_SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_occ_loss_regimes(shape, mask):
    for c in R.occ_cases([shape]):
        if c["mask"] == mask:
            run_occ_case(c)


@pytest.mark.parametrize("shape", R.OCC_LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_occ_loss_grid_edges(shape):
    run_occ_case(dict(B=shape[0], n=shape[1], mask="sparse", logits="normal", resid="normal"))


@pytest.mark.parametrize("mask", ["sparse", "no_res"])
def test_occ_loss_function_gives_the_abi_bits(mask):
    from btcdet_amd.occ_head import OccLossFunction
    c = dict(B=3, n=257, mask=mask, logits="normal", resid="normal")
    d, abi = run_occ_case(c)
    logit = up(d["logit"]).requires_grad_(True)
    res = up(d["res"]).requires_grad_(True) if d["res"] is not None else None
    tgt = up(d["tgt"]) if d["res"] is not None else None
    total, parts = OccLossFunction.apply(logit, res, tgt, up(d["pos"]), up(d["cm"]), up(d["cw"]), up(d["rm"]) if res is not None else None,
                                         up(d["rw"]) if res is not None else None, d["beta"], d["w_cls"], d["w_res"])
    total.backward(torch.tensor(R.G_UP, device=dev()))
    assert bits_equal(total.detach().reshape(1), abi["out"][2:3]) and bits_equal(parts.detach(), abi["out"][:2])
    assert bits_equal(logit.grad, abi["d_logit"])
    if res is not None:
        assert bits_equal(res.grad, abi["d_res"])


@pytest.mark.parametrize("regime", R.OCC_LOGITS)
@pytest.mark.parametrize("shape", R.PROB_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_occ_prob(shape, regime):
    from btcdet_amd._lib import ptr, stream_ptr
    B, n = shape
    logit, mask = R.make_prob(B, n, regime)
    tl, tm = up(logit), up(mask)
    outs = []
    for _ in range(2):
        prob = nan_like((B, n))
        call("btc_occ_prob", ptr(tl), ptr(tm), B, n, ptr(prob), stream_ptr())
        outs.append(prob)
    assert bits_equal(*outs)
    W.check("occ_prob", outs[0].cpu().numpy(), R.occ_prob(logit, mask), f"{B}x{n} {regime}")
    assert not bool(outs[0][tm == 0].any())


# ------------------------------------------------------------------------------------------------------------------ sumsq2
def placed(values, bf16, offset):
    """the values in a tensor that starts `offset` elements behind a 16-byte aligned address (None stays None)"""
    if values is None:
        return None
    dt = torch.bfloat16 if bf16 else torch.float32
    base = torch.zeros((values.size + 16,), dtype=dt, device=dev())
    assert base.data_ptr() % 16 == 0
    v = base[offset:offset + values.size]
    v.copy_(up(values, dt))
    return v


def sumsq_abi(a, ka, b, kb, c, align, ws):
    from btcdet_amd._lib import ptr, stream_ptr
    bfa, bfb = c["ta"] == "bf16", c["tb"] == "bf16"
    ta, tb = placed(a, bfa, align[0]), placed(b, bfb, align[1])
    na, nb = a.size, (b.size if b is not None else 0)
    out = nan_like((1,))
    call("btc_sumsq2_fwd", ptr(ta), na, int(bfa), ka, ptr(tb), nb, int(bfb), kb, ptr(out), ptr(ws), ws.numel(), stream_ptr())
    head_zero(ws, "btc_sumsq2_fwd")
    g = torch.full((1,), R.G_UP, dtype=torch.float32, device=dev())
    da = torch.full_like(ta, float("nan"))
    db = torch.full_like(tb, float("nan")) if tb is not None else None
    call("btc_sumsq2_bwd", ptr(ta), na, int(bfa), float(np.float32(2.0 * ka)), ptr(da), ptr(tb), nb, int(bfb), float(np.float32(2.0 * kb)), ptr(db),
         ptr(g), stream_ptr())
    return dict(out=out, da=da, db=db)


@pytest.mark.parametrize("c", R.sumsq_cases(), ids=lambda c: "-".join(str(v) for v in c.values()))
def test_sumsq2(c):
    from btcdet_amd._lib import lib
    a, b, ka, kb = R.make_sumsq(c)
    ws = dirty_ws(lib().btc_sumsq2_ws_bytes())
    for al in R.SUMSQ_ALIGN:
        if b is None and al[1]:
            continue
        first = sumsq_abi(a, ka, b, kb, c, al, ws)
        again = sumsq_abi(a, ka, b, kb, c, al, ws)
        for k in first:
            assert bits_equal(first[k], again[k]), (k, al)
        got = {k: (v.float().cpu().numpy() if v is not None else None) for k, v in first.items()}
        got["g"] = R.G_UP
        R.check_sumsq(W, a, ka, b, kb, c, got, f"{c} align {al}")


@pytest.mark.parametrize("types", [("fp32", "fp32"), ("bf16", "fp32"), ("bf16", None)], ids=str)
def test_mean_square2_gives_the_abi_bits(types):
    from btcdet_amd._lib import lib
    from btcdet_amd.trainer import MeanSquare2
    c = dict(na=4097, nb=4095 if types[1] else 0, ta=types[0], tb=types[1])
    a, b, ka, kb = R.make_sumsq(c)
    abi = sumsq_abi(a, ka, b, kb, c, (0, 0), dirty_ws(lib().btc_sumsq2_ws_bytes()))
    ta = placed(a, types[0] == "bf16", 0).requires_grad_(True)
    tb = placed(b, types[1] == "bf16", 0).requires_grad_(True) if b is not None else None
    out = MeanSquare2.apply(ta, 1e-3, tb, 1e-3 if b is not None else 0.0)
    out.backward(torch.tensor(R.G_UP, device=dev()))
    assert bits_equal(out.detach().reshape(1), abi["out"]) and bits_equal(ta.grad, abi["da"])
    if tb is not None:
        assert bits_equal(tb.grad, abi["db"])


# ------------------------------------------------------------------------------------------------------------------ adam / grads_pack
def guarded(values):
    """a view, PAD elements into a canary-filled allocation, holding the values -> (view, whole allocation)"""
    whole = torch.full((values.size + 2 * PAD + 27,), CANARY, dtype=torch.float32, device=dev())
    view = whole[PAD:PAD + values.size]
    view.copy_(up(values))
    return view, whole


def canaries_intact(whole, n):
    return bool((whole[:PAD] == CANARY).all()) and bool((whole[PAD + n:] == CANARY).all())


def device_grads(grads):
    """every gradient its own allocation; the odd ones views one element into theirs (4-byte aligned only)"""
    out = []
    for i, x in enumerate(grads):
        if i % 2:
            t = torch.zeros((x.size + 1,), dtype=torch.float32, device=dev())[1:]
            t.copy_(up(x))
            assert t.data_ptr() % 8 == 4
        else:
            t = up(x)
        out.append(t)
    return out


def adam_abi(grads, p0, m0, v0, hp, tabs=None):
    from btcdet_amd._lib import lib, ptr, stream_ptr
    from btcdet_amd.train_step import chunk_tables
    sizes = [x.size for x in grads]
    nt = sum(sizes)
    if tabs is None:
        tabs = chunk_tables(sizes, dev())
        twin = R.chunk_tables_np(sizes, int(lib().btc_adam_max_segments()))
        assert tabs["seg0"] == twin["seg0"] and all(np.array_equal(tabs[k].cpu().numpy(), twin[k]) for k in ("seg", "off", "len", "flat"))
    tg = device_grads(grads)
    gp = (ctypes.c_void_p * len(tg))(*[t.data_ptr() for t in tg])
    c0 = np.array(tabs["seg0"], dtype=np.int32)
    c0p = c0.ctypes.data_as(c_i32p)
    table = (ptr(tabs["seg"]), ptr(tabs["off"]), ptr(tabs["len"]), ptr(tabs["flat"]), c0p)
    packed, packed_all = guarded(np.full(nt, np.nan, np.float32))
    call("btc_grads_pack", gp, len(tg), *table, ptr(packed), stream_ptr())
    nch = int(tabs["seg"].numel())
    ws = torch.full((int(lib().btc_adam_group_ws_bytes(nch)),), 0xFF, dtype=torch.uint8, device=dev())     # nothing of it is promised zero
    (p, pa), (m, ma), (v, va) = guarded(p0), guarded(m0), guarded(v0)
    call("btc_adam_group_step", gp, len(tg), *table, nch, ptr(p), ptr(m), ptr(v), hp["step"], hp["lr"], hp["beta1"], hp["beta2"], hp["eps"],
         hp["wd"], hp["clip"], ptr(ws), ws.numel(), stream_ptr())
    torch.cuda.synchronize()
    for whole in (packed_all, pa, ma, va):
        assert canaries_intact(whole, nt), "a write outside the flat buffer"
    for t, x in zip(tg, grads):
        assert np.array_equal(t.cpu().numpy(), x), "a gradient was modified"
    return dict(packed=packed, p=p, m=m, v=v, tsq=ws[:8].clone().view(torch.float64))


def run_adam_case(c):
    grads, p0, m0, v0, hp = R.make_adam(c)
    first = adam_abi(grads, p0, m0, v0, hp)
    again = adam_abi(grads, p0, m0, v0, hp)
    for k in first:
        if k != "tsq" or hp["clip"] > 0:
            assert bits_equal(first[k], again[k]), f"{k} differs between two identical calls, {R.adam_name(c)}"
    got = {k: v.cpu().numpy() for k, v in first.items()}
    got["tsq"] = float(got["tsq"][0])
    R.check_adam(W, grads, p0, m0, v0, hp, got, R.adam_name(c))
    return grads, p0, m0, v0, hp, first


def _ids(c):
    return R.adam_name(c)


@pytest.mark.parametrize("clip", R.ADAM_CLIPS)
@pytest.mark.parametrize("sizes", R.ADAM_SMALL, ids=lambda s: str(s[0]))
def test_adam_regimes(sizes, clip):
    for c in R.adam_cases():
        if c["sizes"] == sizes and c["clip"] == clip:
            run_adam_case(c)


@pytest.mark.parametrize("c", [c for c in R.adam_cases() if c["sizes"] not in R.ADAM_SMALL], ids=_ids)
def test_adam_launch_and_chunk_loops(c):
    run_adam_case(c)


def test_group_optimizer_and_binding_give_the_abi_bits():
    """GroupOptimizer(flat=True), F.adam_group_step and F.pack_grads on a group of 466 parameters (two launches)"""
    from btcdet_amd import _lib
    from btcdet_amd._lib import stream_ptr
    from btcdet_amd.train_step import GroupOptimizer, chunk_tables
    F = _lib.fast()
    assert F is not None, "the compiled binding is not built"
    c = dict(sizes=[5, 1024, 1025, 1, 3000, 2048] + [7] * 460, clip="biting", zero_grad=False, step=1, wd=0.01, beta1=0.95, moments="zero")
    grads, p0, m0, v0, hp = R.make_adam(c)
    sizes, cuts = c["sizes"], np.cumsum(c["sizes"])[:-1]
    params = [torch.nn.Parameter(up(x)) for x in np.split(p0, cuts)]
    opt = GroupOptimizer([dict(params=params, lr=0.03, weight_decay=hp["wd"], grad_norm_clip=hp["clip"], moms=(0.95, 0.85), div_factor=10.0)], 100, flat=True)
    fl = opt.groups[0].get("flat")
    assert fl is not None, "the flat path was not taken"
    hp = dict(hp, lr=opt.groups[0]["lr"], beta1=opt.groups[0]["mom"])
    abi = adam_abi(grads, p0, m0, v0, hp)
    tg = device_grads(grads)
    for q, g in zip(params, tg):
        q.grad = g
    opt.step()
    assert fl["n"] == 1, "the step left the flat path"
    assert bits_equal(fl["p"], abi["p"].clone()) and bits_equal(fl["m"], abi["m"].clone()) and bits_equal(fl["v"], abi["v"].clone())
    assert bits_equal(fl["ws"][:8].view(torch.float64), abi["tsq"])
    # the binding's own entry points
    t = chunk_tables(sizes, dev())
    p, m, v = up(p0), up(m0), up(v0)
    views = [x.view(-1) for x in torch.split(p, sizes)]
    ws = torch.zeros((int(_lib.lib().btc_adam_group_ws_bytes(int(t["seg"].numel()))),), dtype=torch.uint8, device=dev())
    F.adam_group_step(views, tg, t["seg"], t["off"], t["len"], t["flat"], t["seg0"], p, m, v, 1, float(hp["lr"]), float(hp["beta1"]), 0.99, 1e-8,
                      float(hp["wd"]), float(hp["clip"]), ws, stream_ptr())
    assert bits_equal(p, abi["p"].clone()) and bits_equal(m, abi["m"].clone()) and bits_equal(v, abi["v"].clone())
    flat = nan_like((sum(sizes),))
    F.pack_grads(tg, t["seg"], t["off"], t["len"], t["flat"], t["seg0"], sizes, flat, stream_ptr())
    assert bits_equal(flat, abi["packed"].clone())


# ------------------------------------------------------------------------------------------------------------------ report
def test_report_worst_ratios(capsys):
    """last in the file: the worst ratio to its bound per stage over everything the tests above checked"""
    assert all(r <= 1.0 for r in W.worst.values())
    with capsys.disabled():
        print("\n" + W.report())
