"""btc_anchor_loss_fwd / _bwd (csrc/anchor_loss.hip, include/btcdet_hip_anchor_loss.h) through btcdet_amd.anchor_loss on the GPU: the
golden cases of the reference, shape edges (tile, sweep and grid-cap edges named by the header's constants), value edges and KITTI size
against the float64 restatement of tests/anchor_loss_ref.py inside its DERIVED bound -- the worst ratio |got - ref| / bound is printed per
output; the structure of the two launches (zeros where the labels exclude, every output element written, NaN at excluded inputs changes
no bit, two calls bit-identical, no synchronisation); and the wiring of AnchorHeadSingle.get_loss behind LOSS_CONFIG.DEVICE."""
import logging

import numpy as np
import pytest
import torch

import anchor_loss_ref as al
import anchor_targets_ref as ar

pytestmark = pytest.mark.gpu
G, CASES = al.gold()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(d, g=al.G_UP):
    """one forward and one backward through btcdet_amd.anchor_loss -> the dict check_anchor takes"""
    from btcdet_amd import anchor_loss
    cls, box = _dev(d["cls"]).requires_grad_(True), _dev(d["box"]).requires_grad_(True)
    dirs = _dev(d["dir"]).requires_grad_(True) if d["dir"] is not None else None
    total, parts = anchor_loss.anchor_loss(cls, box, dirs, _dev(d["labels"]), _dev(d["tgt"]), _dev(d["anchors"]), d["w"], d["dir_offset"])
    assert not parts.requires_grad and total.requires_grad
    norms = total.grad_fn.saved_tensors[-1].clone()                          # what the forward kept for the backward
    total.backward(torch.tensor(g, dtype=torch.float32, device="cuda"))
    out = parts.cpu().numpy()
    assert float(total.detach()) == float(out[3])
    return dict(out=out, norms=norms.cpu().numpy(), d_cls=cls.grad.cpu().numpy(), d_box=box.grad.cpu().numpy(),
                d_dir=dirs.grad.cpu().numpy() if dirs is not None else None, g=g)


def _check(d, where):
    W = al.Worst()
    al.check_anchor(W, d, run(d), where)
    print(where, W.report())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_golden_cases(case):
    d = al.gold_case(G, case["name"], case["dir"])
    _check(d, case["name"])
    if case["f64"]:                                  # and directly against the reference's float64 record, inside the same bound
        got, R = run(d, g=1.0), al.restate(d, norms_k=None, g=1.0)
        bd = al.bounds(al.restate(d, norms_k=got["norms"], g=1.0))
        ref = G[case["name"] + "/loss64"]
        for q, name in enumerate(("out_cls", "out_loc", "out_dir")):
            assert abs(float(got["out"][q]) - ref[q]) <= bd[name][1][0] + 1e-12 * abs(ref[q]), name
        for key in ("d_cls", "d_box") + (("d_dir",) if case["dir"] else ()):
            assert al.ratio(got[key], G[case["name"] + "/" + key + "64"], bd[key][1] + 1e-12 * np.abs(R[key])) <= 1.0, key


@pytest.mark.parametrize("case", al.shape_cases(), ids=al.case_name)
def test_shape_edges(case):
    _check(al.make_case(case), al.case_name(case))


@pytest.mark.parametrize("case", al.cap_cases(), ids=al.case_name)
def test_grid_cap_edges(case):
    """one below, at and above what one sweep of the capped grid covers (MAX_TILES * THREADS anchors of a scene), and a ragged second sweep"""
    from btcdet_amd import _lib
    assert _lib.lib().btc_anchor_loss_ws_bytes(case["B"], case["A"]) == 256 + case["B"] * min(-(-case["A"] // al.THREADS), al.MAX_TILES) * 32
    _check(al.make_case(case), al.case_name(case))


@pytest.mark.parametrize("case", al.value_cases(), ids=al.case_name)
def test_value_edges(case):
    _check(al.make_case(case), al.case_name(case))


def test_kitti_size():
    """B = 2, A = 70 400: 550 workgroups, a grid that spans all eight XCDs"""
    _check(al.make_case(al.KITTI_CASE), al.case_name(al.KITTI_CASE))


# ------------------------------------------------------------------------------------------------------------------------ structure
def _raw(d, fill, g=al.G_UP):
    """both entry points through ctypes with outputs pre-filled with `fill` -> out, norms, d_cls, d_box, d_dir as device tensors"""
    from btcdet_amd import _lib
    L = _lib.lib()
    B, A, C = d["cls"].shape
    bins = 0 if d["dir"] is None else d["dir"].shape[2]
    t = {k: _dev(d[k]) for k in ("cls", "box", "labels", "tgt", "anchors")}
    t["dir"] = _dev(d["dir"]) if bins else None
    p = lambda x: None if x is None else x.data_ptr()
    full = lambda *s: torch.full(s, fill, dtype=torch.float32, device="cuda")
    out, norms, d_cls, d_box, d_dir = full(4), full(B), full(B, A, C), full(B, A, 7), (full(B, A, bins) if bins else None)
    ws_bytes = L.btc_anchor_loss_ws_bytes(B, A)
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    ws[:256] = 0
    gup = torch.tensor([g], dtype=torch.float32, device="cuda")
    w = d["w"]
    args = (p(t["cls"]), p(t["box"]), p(t["dir"]), p(t["labels"]), p(t["tgt"]), p(t["anchors"]), B, A, C, bins, w["cls_weight"], w["loc_weight"],
            w["dir_weight"] if bins else 0.0, d["dir_offset"])
    _lib.check(L.btc_anchor_loss_fwd(*args, p(out), p(norms), p(ws), ws_bytes, _lib.stream_ptr()), "btc_anchor_loss_fwd")
    _lib.check(L.btc_anchor_loss_bwd(*args, p(norms), p(gup), p(d_cls), p(d_box), p(d_dir), _lib.stream_ptr()), "btc_anchor_loss_bwd")
    torch.cuda.synchronize()
    assert bool((ws[:256] == 0).all()), "the workspace head is left zero"
    return [out, norms, d_cls, d_box] + ([d_dir] if bins else [])


def _bits(a, b):
    return torch.equal(a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32))


@pytest.mark.parametrize("case", [dict(B=3, A=513, C=3, bins=2, kind="random"), dict(B=2, A=257, C=1, bins=0, kind="nan_target")], ids=al.case_name)
def test_excluded_entries_and_full_overwrite(case):
    poisoned, zeros = al.make_case(case, poison=True), al.make_case(case, poison=False)
    a, b, c = _raw(poisoned, float("nan")), _raw(zeros, 7.0), _raw(poisoned, float("nan"))
    for x, y, z in zip(a, b, c):
        assert not bool(torch.isnan(x).any()), "an output allocated as NaN is fully overwritten"
        assert _bits(x, y), "NaN at excluded predictions and targets changes no output bit against zeros there"
        assert _bits(x, z), "two calls on the same inputs give the same bits"
    labels = _dev(poisoned["labels"])
    assert not bool(a[2][labels < 0].any()) and not bool(a[3][labels <= 0].any()) and (len(a) == 4 or not bool(a[4][labels <= 0].any()))


def test_no_synchronisation():
    from btcdet_amd import anchor_loss
    d = al.make_case(dict(B=2, A=1030, C=3, bins=2, kind="random"))
    cls, box, dirs = (_dev(d[k]).requires_grad_(True) for k in ("cls", "box", "dir"))
    labels, tgt, anchors = _dev(d["labels"]), _dev(d["tgt"]), _dev(d["anchors"])
    g = torch.tensor(al.G_UP, device="cuda")
    anchor_loss.anchor_loss(cls, box, dirs, labels, tgt, anchors, d["w"], d["dir_offset"])[0].backward(g)        # the workspace exists now
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, parts = anchor_loss.anchor_loss(cls, box, dirs, labels, tgt, anchors, d["w"], d["dir_offset"])
        total.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(parts).all())


# --------------------------------------------------------------------------------------------------------------------------- wiring
def _head(cfg):
    from btcdet_amd.dense_head import AnchorHeadSingle
    m = al.GOLD_MAPS["car"]
    torch.manual_seed(3)
    return AnchorHeadSingle(cfg, input_channels=8, num_class=1, class_names=m["class_names"], grid_size=np.array(m["grid_size"]),
                            point_cloud_range=np.array(m["point_cloud_range"], np.float32)).cuda().train()


def _step(head, x, gt):
    head.zero_grad()
    head(dict(spatial_features_2d=x, gt_boxes=gt.clone(), batch_size=int(x.shape[0])))
    loss, tb = head.get_loss()
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {k: float(v) for k, v in tb.items()}, {n: p.grad.cpu().numpy().astype(np.float64) for n, p in head.named_parameters()}


def test_head_routes_agree():
    """an AnchorHeadSingle with LOSS_CONFIG.DEVICE and one without, on the same weights and inputs.  Both lie inside the bound around the
    float64 values, so they differ by at most twice the bound: the losses, and the prediction gradients per element.  A parameter gradient
    of a 1x1 conv is sum over (scene, location) of d_out * x -- fp32 accumulation by the vendor's kernel, order unknown: the tolerance is
    sum 2 bound(d_out) |x| + 2^-20 sum |d_out x| (2^-20: sixteen times u for a sum of B * 64 = 192 terms in any order)"""
    from btcdet_amd.dense_head import AnchorHeadSingle
    plain, fused = _head(al.gold_cfg("car")), _head(al.gold_cfg("car", DEVICE=True))
    fused.load_state_dict(plain.state_dict())
    assert fused.device_loss and not plain.device_loss
    rng = np.random.default_rng(11)
    B = 3
    x = _dev(rng.standard_normal((B, 8, 8, 8)).astype(np.float32))
    gt = np.stack([ar.random_boxes(rng, 3, 1, (1, -7, 15, 7), pad=1) for _ in range(B)])
    gt[1] = 0                                        # a scene without a box
    la, ta, ga = _step(plain, x, _dev(gt))
    lb, tb, gb = _step(fused, x, _dev(gt))
    assert list(ta) == list(tb) == ["rpn_loss_cls", "rpn_loss_loc", "rpn_loss_dir", "rpn_loss"]
    f = fused.forward_ret_dict
    A = f["box_cls_labels"].shape[1]
    d = dict(cls=f["cls_preds"].detach().cpu().numpy().reshape(B, A, 1), box=f["box_preds"].detach().cpu().numpy().reshape(B, A, 7),
             dir=f["dir_cls_preds"].detach().cpu().numpy().reshape(B, A, 2), labels=f["box_cls_labels"].cpu().numpy(), tgt=f["box_reg_targets"].cpu().numpy(),
             anchors=torch.cat(fused.anchors("cuda"), dim=-3).reshape(-1, 7).cpu().numpy(), w=dict(al.W_DEFAULT), dir_offset=al.DIR_OFFSET)
    assert (d["labels"] > 0).any() and (d["labels"][1] == 0).all()
    R = al.restate(d)
    bd = al.bounds(R)
    for q, (key, name) in enumerate((("rpn_loss_cls", "out_cls"), ("rpn_loss_loc", "out_loc"), ("rpn_loss_dir", "out_dir"))):
        assert abs(ta[key] - tb[key]) <= 2 * bd[name][1][0], (key, ta[key], tb[key])
    assert abs(la - lb) <= 2 * sum(bd[n][1][0] for n in ("out_cls", "out_loc", "out_dir")) + 2.0 ** -22 * abs(la)
    xs = x.cpu().numpy().astype(np.float64)                                   # (B, 8 in, 8, 8)
    for conv, key, width in (("conv_cls", "d_cls", 1), ("conv_box", "d_box", 7), ("conv_dir_cls", "d_dir", 2)):
        ref, bound = (v.reshape(B, 8, 8, 2 * width) for v in bd[key])         # per location: the slots' columns = the conv's output channels
        tol_w = np.einsum("byxo,biyx->oi", 2 * bound, np.abs(xs)) + 2.0 ** -20 * np.einsum("byxo,biyx->oi", np.abs(ref), np.abs(xs))
        tol_b = (2 * bound).sum((0, 1, 2)) + 2.0 ** -20 * np.abs(ref).sum((0, 1, 2))
        dw, db = np.abs(ga[conv + ".weight"] - gb[conv + ".weight"])[:, :, 0, 0], np.abs(ga[conv + ".bias"] - gb[conv + ".bias"])
        print(conv, "worst parameter-gradient difference / tolerance: weight %.3f bias %.3f" % ((dw / tol_w).max(), (db / tol_b).max()))
        assert np.all(dw <= tol_w) and np.all(db <= tol_b), conv
        assert np.abs(gb[conv + ".weight"]).max() > 0


def test_unsupported_and_cpu_keep_the_torch_route(caplog, monkeypatch):
    from btcdet_amd import anchor_loss
    cfg = al.gold_cfg("car", DEVICE=True)
    cfg.NUM_DIR_BINS = 17
    with caplog.at_level(logging.WARNING, logger="btcdet_amd.dense_head"):
        h = _head(cfg)
    assert not h.device_loss and any("NUM_DIR_BINS" in r.getMessage() for r in caplog.records)
    calls = []
    real = anchor_loss.anchor_loss
    monkeypatch.setattr(anchor_loss, "anchor_loss", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((2, 8, 8, 8)).astype(np.float32))
    gt = torch.from_numpy(np.stack([ar.random_boxes(rng, 2, 1, (1, -7, 15, 7), pad=1) for _ in range(2)]))
    keyed = _head(al.gold_cfg("car", DEVICE=True))
    _step(keyed, x.cuda(), gt.cuda())
    assert calls == [1], "GPU tensors take the fused route"
    _step(keyed.cpu(), x, gt)
    assert calls == [1], "CPU tensors keep the torch route"
