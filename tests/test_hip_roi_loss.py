"""btc_roi_loss_fwd / _bwd (csrc/roi_loss.hip, include/btcdet_hip_roi_loss.h) through btcdet_amd.roi_loss on the GPU: the golden cases of the
reference, shape edges (tile, sweep and grid-cap edges named by the header's constants), value edges, KITTI size and one large N against
the restatement of tests/roi_loss_ref.py inside its DERIVED bound -- the worst ratio |got - ref| / bound is printed per output; the
structure of the two launches (zeros where the labels and the mask exclude, every output element written, NaN at excluded inputs changes
no bit, two calls bit-identical, the workspace head left zero, no synchronisation); and the wiring of ConvHead.get_loss behind
ROI_HEAD.LOSS_CONFIG.DEVICE."""
import copy
import logging

import numpy as np
import pytest
import torch

import roi_loss_ref as rl

pytestmark = pytest.mark.gpu
G, CASES = rl.gold()
KEYS = ("rcnn_cls", "rcnn_reg", "rois", "gt_of_rois", "gt_of_rois_src", "reg_valid_mask", "rcnn_cls_labels")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ret(d):
    """a case dict as the head's forward_ret_dict, on the device (one scene: the kernels take the rois flat)"""
    N = d["mask"].size
    return dict(rcnn_cls=_dev(d["cls"]).view(N, 1).requires_grad_(True), rcnn_reg=_dev(d["reg"]).view(N, 7).requires_grad_(True),
                rois=_dev(d["rois"]).view(1, N, 7), gt_of_rois=_dev(d["gt"]).view(1, N, -1) if N else _dev(d["gt"]).view(1, 0, 8),
                gt_of_rois_src=_dev(d["src"]).view(1, N, -1) if N else _dev(d["src"]).view(1, 0, 8), reg_valid_mask=_dev(d["mask"]).view(1, N),
                rcnn_cls_labels=_dev(d["labels"]).view(1, N))


def run(d, g=rl.G_UP):
    """one forward and one backward through btcdet_amd.roi_loss -> the dict check_roi takes"""
    from btcdet_amd import roi_loss
    ret = _ret(d)
    total, parts = roi_loss.roi_loss(ret, d["w"], d["corner"])
    assert not parts.requires_grad and total.requires_grad
    norms = total.grad_fn.saved_tensors[-1].clone()                          # what the forward kept for the backward
    total.backward(torch.tensor(g, dtype=torch.float32, device="cuda"))
    out = parts.cpu().numpy()
    assert float(total.detach()) == float(out[4])
    return dict(out=out, norms=norms.cpu().numpy(), d_cls=ret["rcnn_cls"].grad.cpu().numpy().reshape(-1), d_reg=ret["rcnn_reg"].grad.cpu().numpy(), g=g)


def _check(d, where):
    W = rl.Worst()
    got = run(d)
    rl.check_roi(W, d, got, where)
    print(where, W.report())
    return got


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_golden_cases(case):
    d = rl.gold_case(G, case["name"], case["corner"])
    _check(d, case["name"])
    # and directly against the reference's float64 record, inside the same bound
    got = run(d, g=1.0)
    bd, R = rl.bounds(d, norms_k=got["norms"], g=1.0)
    ref = G[case["name"] + "/loss64"]
    for q, name in enumerate(("out_cls", "out_reg", "out_corner")):
        assert abs(float(got["out"][q]) - ref[q]) <= bd[name][1][0] + 1e-12 * abs(ref[q]), name
    for key in ("d_cls", "d_reg"):
        assert rl.ratio(got[key], G[case["name"] + "/" + key + "64"], bd[key][1] + 1e-12 * np.abs(R[key])) <= 1.0, key


@pytest.mark.parametrize("case", rl.shape_cases(), ids=rl.case_name)
def test_shape_edges(case):
    """N = 0 and 1, one tile - 1, one tile, one tile + 1, two tiles + 3 (BTC_ROI_LOSS_TILE rois per workgroup)"""
    got = _check(rl.make_case(case), rl.case_name(case))
    if case["N"] == 0:
        assert np.array_equal(got["out"], np.zeros(5, np.float32)) and np.array_equal(got["norms"], np.ones(2, np.float32))


@pytest.mark.parametrize("case", rl.cap_cases(), ids=rl.case_name)
def test_grid_cap_edges(case):
    """one below, at and above what one sweep of the capped grid covers (BTC_ROI_LOSS_MAX_TILES * BTC_ROI_LOSS_TILE rois)"""
    from btcdet_amd import _lib
    assert _lib.lib().btc_roi_loss_ws_bytes(case["N"]) == 256 + min(-(-case["N"] // rl.TILE), rl.MAX_TILES) * 40
    _check(rl.make_case(case), rl.case_name(case))


@pytest.mark.parametrize("case", rl.value_cases(), ids=rl.case_name)
def test_value_edges(case):
    _check(rl.make_case(case), rl.case_name(case))


def test_kitti_size():
    """ROI_PER_IMAGE 128, batch size 2"""
    _check(rl.make_case(rl.KITTI_CASE), rl.case_name(rl.KITTI_CASE))


def test_large_n():
    """a ragged third sweep of the capped grid, int64 labels"""
    _check(rl.make_case(rl.LARGE_CASE), rl.case_name(rl.LARGE_CASE))


def test_saturated_class_terms_are_exact():
    """one valid roi, so out[0] is the term itself: 100 (1 - t) cls_weight where p rounds to 1.0f, 100 t cls_weight where p underflows, and
    a gradient of exactly 0 where p rounds to 1.0f"""
    for x, t, want in ((17.0, 0.25, 75.0), (20.0, 0.0, 100.0), (120.0, 1.0, 0.0), (120.0, 0.5, 50.0), (-104.0, 0.75, 75.0), (-104.0, 0.0, 0.0)):
        d = rl.make_case(dict(N=1, kind="random", labels="roi_iou", corner=False))
        d["cls"], d["labels"] = np.array([x], np.float32), np.array([t], np.float32)
        got = run(d)
        assert float(got["out"][0]) == want * rl.W_DEFAULT["rcnn_cls_weight"], (x, t, got["out"])
        assert x < 0 or float(got["d_cls"][0]) == 0.0, (x, t, got["d_cls"])
        assert abs(float(got["d_cls"][0])) < 1e-30


# ------------------------------------------------------------------------------------------------------------------------ structure
def _raw(d, fill, g=rl.G_UP):
    """both entry points through ctypes with outputs pre-filled with `fill` -> out, norms, d_cls, d_reg as device tensors"""
    from btcdet_amd import _lib
    L = _lib.lib()
    N = d["mask"].size
    t = {k: _dev(d[k]) for k in ("cls", "reg", "rois", "gt", "src", "mask", "labels")}
    p = lambda x: x.data_ptr() if N else None
    full = lambda *s: torch.full(s, fill, dtype=torch.float32, device="cuda")
    out, norms, d_cls, d_reg = full(5), full(2), full(N), full(N, 7)
    ws_bytes = L.btc_roi_loss_ws_bytes(N)
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    ws[:256] = 0
    gup = torch.tensor([g], dtype=torch.float32, device="cuda")
    w = d["w"]
    args = (p(t["cls"]), p(t["reg"]), p(t["rois"]), p(t["gt"]), p(t["src"]), 8, p(t["mask"]), p(t["labels"]), rl.kind_of(d), N, int(d["corner"]),
            w["rcnn_cls_weight"], w["rcnn_reg_weight"], w["rcnn_corner_weight"])
    _lib.check(L.btc_roi_loss_fwd(*args, out.data_ptr(), norms.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr()), "btc_roi_loss_fwd")
    _lib.check(L.btc_roi_loss_bwd(*args, norms.data_ptr(), gup.data_ptr(), p(d_cls), p(d_reg), _lib.stream_ptr()), "btc_roi_loss_bwd")
    torch.cuda.synchronize()
    assert bool((ws[:256] == 0).all()), "the workspace head is left zero"
    return [out, norms, d_cls, d_reg]


def _bits(a, b):
    return torch.equal(a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32))


@pytest.mark.parametrize("case", [dict(N=2 * rl.TILE + 3, kind="random", labels="cls", corner=True), dict(N=rl.VALUE_N, kind="nan_target", labels="roi_iou", corner=True),
                                  dict(N=rl.VALUE_N, kind="fg_ignored", labels="cls", corner=False)], ids=rl.case_name)
def test_excluded_entries_and_full_overwrite(case):
    poisoned, zeros = rl.make_case(case, poison=True), rl.make_case(case, poison=False)
    assert np.isnan(poisoned["reg"]).any() and np.isnan(poisoned["cls"]).any() == (case["labels"] == "cls")
    a, b, c = _raw(poisoned, float("nan")), _raw(zeros, 7.0), _raw(poisoned, float("nan"))
    for x, y, z in zip(a, b, c):
        assert not bool(torch.isnan(x).any()), "an output allocated as NaN is fully overwritten"
        assert _bits(x, y), "NaN at excluded predictions, rois and boxes changes no output bit against zeros there"
        assert _bits(x, z), "two calls on the same inputs give the same bits"
    assert not bool(a[2][_dev(poisoned["labels"]) < 0].any()) and not bool(a[3][_dev(poisoned["mask"]) <= 0].any())


def test_no_synchronisation():
    from btcdet_amd import roi_loss
    d = rl.make_case(dict(N=3 * rl.TILE + 5, kind="random", labels="roi_iou", corner=True))
    ret = _ret(d)
    g = torch.tensor(rl.G_UP, device="cuda")
    roi_loss.roi_loss(ret, d["w"], True)[0].backward(g)                     # the workspace exists now
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, parts = roi_loss.roi_loss(ret, d["w"], True)
        total.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(parts).all())


# --------------------------------------------------------------------------------------------------------------------------- wiring
def _head(device_key=None, **loss_extra):
    from btcdet_amd.config import load_cfg
    from btcdet_amd.conv_head import ConvHead
    from btcdet_amd.dense_head import ResidualCoder
    cfg = copy.deepcopy(load_cfg().MODEL.ROI_HEAD)
    cfg.LOSS_CONFIG.LOSS_WEIGHTS.update(rl.W_DEFAULT)
    for k, v in loss_extra.items():
        cfg.LOSS_CONFIG[k] = v
    if device_key is not None:
        cfg.LOSS_CONFIG["DEVICE"] = device_key
    head = ConvHead.__new__(ConvHead)
    torch.nn.Module.__init__(head)
    head.model_cfg, head.box_coder = cfg, ResidualCoder()
    return head


def _targets(route, seed=0):
    """targets of one hand-made batch: rois scattered around the boxes, B = 2, through either assign_targets route"""
    from btcdet_amd.config import load_cfg
    from btcdet_amd.conv_head import ConvHead
    rng = np.random.default_rng(seed)
    B, Nr, Gb = 2, 160, 6
    gt = np.zeros((B, Gb, 8), np.float32)
    for b in range(B):
        n = 4 + b
        gt[b, :n] = np.concatenate([rng.uniform(5, 40, (n, 1)), rng.uniform(-15, 15, (n, 1)), rng.uniform(-1.5, -0.5, (n, 1)), rng.uniform(3.2, 4.5, (n, 1)),
                                    rng.uniform(1.5, 1.9, (n, 1)), rng.uniform(1.4, 1.7, (n, 1)), rng.uniform(-3, 3, (n, 1)), np.ones((n, 1))], 1)
    pick = rng.integers(0, 4, (B, Nr))
    rois = np.stack([gt[b, pick[b], :7] for b in range(B)])
    rois = rois + rng.standard_normal(rois.shape).astype(np.float32) * np.array([0.5, 0.5, 0.15, 0.2, 0.1, 0.1, 0.15], np.float32) * rng.random((B, Nr, 1)).astype(np.float32) * 2
    rois[:, ::7, 6] += np.where(rois[:, ::7, 6] > 0, -np.pi, np.pi).astype(np.float32)   # some proposals face the other way
    cfg = copy.deepcopy(load_cfg().MODEL.ROI_HEAD)
    if route == "device":
        cfg.TARGET_CONFIG["DEVICE"] = True
    head = ConvHead.__new__(ConvHead)
    torch.nn.Module.__init__(head)
    head.model_cfg = cfg
    bd = dict(rois=_dev(rois.astype(np.float32)), roi_scores=_dev(rng.random((B, Nr)).astype(np.float32)), roi_labels=torch.ones((B, Nr), dtype=torch.int64, device="cuda"),
              gt_boxes=_dev(gt), batch_size=B)
    t = head.assign_targets(bd)
    assert ("max_overlaps" in t) == (route == "device")
    return t


@pytest.mark.parametrize("route", ["device", "torch"])
def test_head_routes_agree(route):
    """two ConvHeads with and without the key on one hand-made forward_ret_dict whose targets come from DeviceProposalTargets or from
    ProposalTargetLayer + canonical_targets.  Both routes lie inside the bound around the float64 values, so they differ by at most twice
    the bound: the losses, and the prediction gradients per element"""
    t = _targets(route)
    B, R = t["rois"].shape[:2]
    N = B * R
    rng = np.random.default_rng(3)
    cls0 = _dev(np.clip(rng.standard_normal((N, 1)) * 2, -6, 6).astype(np.float32))
    reg0 = _dev((rng.standard_normal((N, 7)) * np.array([0.2, 0.2, 0.2, 0.1, 0.1, 0.1, 0.15])).astype(np.float32))
    res = []
    for head in (_head(), _head(True)):
        f = dict(t, rcnn_cls=cls0.clone().requires_grad_(True), rcnn_reg=reg0.clone().requires_grad_(True))
        head.forward_ret_dict = f
        loss, tb = head.get_loss()
        loss.backward()
        torch.cuda.synchronize()
        res.append((float(loss.detach()), {k: float(v) for k, v in tb.items()}, f["rcnn_cls"].grad.cpu().numpy().reshape(-1), f["rcnn_reg"].grad.cpu().numpy(), head.device_loss))
    (la, ta, ca, ra, fa), (lb, tb_, cb, rb, fb) = res
    assert fb and not fa
    assert list(ta) == list(tb_) == ["rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss", "rcnn_loss_corner"]
    d = dict(cls=cls0.cpu().numpy().reshape(-1), reg=reg0.cpu().numpy(), rois=t["rois"].cpu().numpy().reshape(N, 7), gt=t["gt_of_rois"].cpu().numpy().reshape(N, 8),
             src=t["gt_of_rois_src"].cpu().numpy().reshape(N, 8), mask=t["reg_valid_mask"].cpu().numpy().reshape(N), labels=t["rcnn_cls_labels"].cpu().numpy().reshape(N),
             w=dict(rl.W_DEFAULT), corner=True, B=B)
    m = rl.assert_margins(d)
    assert (d["mask"] > 0).sum() >= 8 and d["labels"].dtype == np.float32, "the hand-made batch has foreground rois"
    bd, Rr = rl.bounds(d)
    b_cls, b_reg, b_cor = (bd[n][1][0] for n in ("out_cls", "out_reg", "out_corner"))
    assert abs(ta["rcnn_loss_cls"] - tb_["rcnn_loss_cls"]) <= 2 * b_cls
    assert abs(ta["rcnn_loss_corner"] - tb_["rcnn_loss_corner"]) <= 2 * b_cor
    assert abs(ta["rcnn_loss_reg"] - tb_["rcnn_loss_reg"]) <= 2 * (b_reg + b_cor) + 2.0 ** -22 * abs(ta["rcnn_loss_reg"])
    assert abs(la - lb) <= 2 * (b_cls + b_reg + b_cor) + 2.0 ** -21 * abs(la)
    assert abs(tb_["rcnn_loss_cls"] - Rr["out"][0]) <= b_cls and abs(tb_["rcnn_loss_reg"] - Rr["out"][3]) <= b_reg + b_cor + 2.0 ** -23 * abs(Rr["out"][3])
    r_cls, r_reg = rl.ratio(ca, cb, 2 * bd["d_cls"][1]), rl.ratio(ra, rb, 2 * bd["d_reg"][1])
    print(route, "tie margin %.3g" % m["tie"], "worst route difference / (2 bound): d_cls %.3f d_reg %.3f" % (r_cls, r_reg))
    assert r_cls <= 1.0 and r_reg <= 1.0 and np.abs(rb).max() > 0 and np.abs(cb).max() > 0


def test_unsupported_and_cpu_keep_the_torch_route(caplog, monkeypatch):
    from btcdet_amd import roi_loss
    calls = []
    real = roi_loss.roi_loss
    monkeypatch.setattr(roi_loss, "roi_loss", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    d = rl.gold_case(G, CASES[0]["name"])
    N = d["mask"].size

    def step(head, device, labels=None):
        t = lambda a, *s: torch.from_numpy(np.ascontiguousarray(a)).view(*s).to(device)
        head.forward_ret_dict = dict(rois=t(d["rois"], 2, N // 2, 7), gt_of_rois=t(d["gt"], 2, N // 2, 8), gt_of_rois_src=t(d["src"], 2, N // 2, 8),
                                     reg_valid_mask=t(d["mask"], 2, N // 2), rcnn_cls_labels=t(d["labels"], 2, N // 2) if labels is None else labels.to(device),
                                     rcnn_cls=t(d["cls"], N, 1).requires_grad_(True), rcnn_reg=t(d["reg"], N, 7).requires_grad_(True))
        loss, tb = head.get_loss()
        loss.backward()
        return float(loss.detach())
    keyed = _head(True)
    a = step(keyed, "cuda")
    assert calls == [1], "GPU tensors take the fused route"
    b = step(keyed, "cpu")
    assert calls == [1] and abs(a - b) < 1e-4 * abs(b), "CPU tensors keep the torch route"
    bad = _head(True, CLS_LOSS="CrossEntropy")
    with caplog.at_level(logging.WARNING, logger="btcdet_amd.conv_head"):
        step(bad, "cuda", labels=torch.zeros((2, N // 2), dtype=torch.int64))
    assert calls == [1] and not bad.device_loss and any("CLS_LOSS" in r.getMessage() for r in caplog.records)
    step(_head(), "cuda")
    assert calls == [1], "without the key the symbol is not touched"


def test_full_heads_step_with_the_key_trains(monkeypatch):
    """one --heads full-shaped forward, loss and backward with ROI_HEAD.TARGET_CONFIG.DEVICE and ROI_HEAD.LOSS_CONFIG.DEVICE: finite, every
    ROI-head parameter gets a gradient, and the loss came from btc_roi_loss_fwd"""
    import bench
    from btcdet_amd import roi_loss
    from btcdet_amd.btc_path import BtcHotPath
    from btcdet_amd.config import load_cfg
    calls = []
    real = roi_loss.roi_loss
    monkeypatch.setattr(roi_loss, "roi_loss", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    cfg = copy.deepcopy(load_cfg())
    cfg.MODEL.ROI_HEAD.TARGET_CONFIG["DEVICE"] = True
    cfg.MODEL.ROI_HEAD.LOSS_CONFIG["DEVICE"] = True
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = BtcHotPath(cfg, device=dev, heads="full").to(dev).train()
    batches = bench.build_batches(2, 0, dev)
    out, tb, bd = model(model.prepare(batches[0]))
    loss = model.det_loss(out, bd) + out["loss_occ"]
    loss.backward()
    assert torch.isfinite(loss) and calls == [1]
    head = model.det_modules.roi_head
    missing = [n for n, p in head.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not missing and head.device_loss, missing
