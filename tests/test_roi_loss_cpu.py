"""btcdet_amd/roi_loss.py without a GPU: the restatement of include/btcdet_hip_roi_loss.h (roi_loss_ref.restate) against the reference's own
float64 record (tests/golden/roi_loss.npz, made by gen_roi_loss_golden.py) at 1e-12 relative; the reference's float32 record, the torch
route of conv_head.ConvHead.get_loss on the CPU and a float32 emulation of the kernels inside the derived bound; seven seeded defects,
each caught on a listed case; unsupported_reason, the opt-in key, the ctypes table against the header and the refusals that need no
launch."""
import copy
import logging
import os
import re

import numpy as np
import pytest
import torch

import roi_loss_ref as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, CASES = rl.gold()


def _gold(case):
    return rl.gold_case(G, case["name"], case["corner"])


def _record(case, suffix):
    n = case["name"]
    return G[n + "/loss" + suffix], G[n + "/d_cls" + suffix], G[n + "/d_reg" + suffix]


def _as_got(d, loss3, d_cls, d_reg, g=1.0):
    """a route's three terms and gradients in the shape check_roi takes: the sums and the normalisers as float32 arithmetic gives them"""
    o = np.asarray(loss3, np.float32)
    o3 = o[1] + o[2]
    nv, nf = max(int((d["labels"] >= 0).sum()), 1), max(int((d["mask"] > 0).sum()), 1)
    return dict(out=np.array([o[0], o[1], o[2], o3, o[0] + o3], np.float32), norms=np.array([1.0 / nv, 1.0 / nf]).astype(np.float32),
                d_cls=d_cls, d_reg=d_reg, g=g)


def test_golden_cases_cover_what_they_must():
    names = {c["name"]: c for c in CASES}
    fg = {n: int((G[n + "/mask"] > 0).sum()) for n in names}
    assert {c["corner"] for c in CASES} == {True, False} and {c["B"] for c in CASES} == {1, 2, 3}
    assert any(v == 0 for v in fg.values()) and any(fg[n] == G[n + "/mask"].size for n in names)
    assert all(G[n + "/mask"].size <= 64 and np.abs(G[n + "/cls"]).max() <= 6 for n in names)
    assert all(G[n + "/labels"].dtype == np.float32 and G[n + "/labels"].min() >= 0 and G[n + "/labels"].max() <= 1 for n in names)
    assert any(np.isnan(G[n + "/gt"][G[n + "/mask"] > 0][:, :7]).any() for n in names), "a NaN regression target at a foreground roi"
    assert any((G[n + "/rois"][G[n + "/mask"] > 0][:, 3:6] < 1e-5).any() for n in names), "roi dims below the clamp"
    assert any((G[n + "/gt"][G[n + "/mask"] > 0][:, 3:6] < 1e-5).any() for n in names), "box dims below the clamp"
    sides = set()
    for c in CASES:                                               # the margins the generator asserted, again on what was recorded
        d = _gold(c)
        rl.assert_margins(d)
        R = rl.restate(d)
        if c["corner"] and R["fg"].any():
            sides |= set((R["m"][R["fg"]] < 1).reshape(-1).tolist())
            assert c["kind"] != "twin_nearer" or (R["ties"][R["fg"]] > 0).all()
    assert sides == {True, False}, "corner distances on both sides of 1"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_restatement_equals_the_float64_record(case):
    R = rl.restate(_gold(case), own=True)
    for got, ref in zip((R["out"][:3], R["d_cls"], R["d_reg"]), _record(case, "64")):
        assert ref.dtype == np.float64 and np.isfinite(ref).all()
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_float32_record_lies_inside_the_bound(case):
    d = _gold(case)
    W = rl.Worst()
    rl.check_roi(W, d, _as_got(d, *_record(case, "32")), case["name"])
    print(case["name"], W.report())


def _head(device_key=None, **loss_extra):
    """a ConvHead that only computes its loss: the configured LOSS_CONFIG with the weights of the case lists"""
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


def _fill(head, d, B, device="cpu"):
    N = d["mask"].size
    t = lambda a, *shape: torch.from_numpy(np.ascontiguousarray(a)).view(*shape).to(device)
    head.forward_ret_dict = dict(rois=t(d["rois"], B, N // B, 7), gt_of_rois=t(d["gt"], B, N // B, 8), gt_of_rois_src=t(d["src"], B, N // B, 8),
                                 reg_valid_mask=t(d["mask"], B, N // B), rcnn_cls_labels=t(d["labels"], B, N // B),
                                 rcnn_cls=t(d["cls"], N, 1).requires_grad_(True), rcnn_reg=t(d["reg"], N, 7).requires_grad_(True))
    return head.forward_ret_dict


def _route(head, d, B, device="cpu"):
    """get_loss + backward -> (the three terms, d_cls, d_reg, the tb_dict's keys, the loss)"""
    f = _fill(head, d, B, device)
    loss, tb = head.get_loss()
    loss.backward()
    tb = {k: float(v) for k, v in tb.items()}
    corner = tb.get("rcnn_loss_corner", 0.0)
    terms = [tb["rcnn_loss_cls"], np.float32(tb["rcnn_loss_reg"]) - np.float32(corner), corner]
    return terms, f["rcnn_cls"].grad.cpu().numpy().reshape(-1), f["rcnn_reg"].grad.cpu().numpy(), list(tb), float(loss.detach()), tb


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_torch_route_on_cpu_lies_inside_the_bound(case):
    """the route the fused one replaces, on the recorded inputs: its gradients and its class term inside the bound; it logs rcnn_loss_reg
    with the corner term added, so regression and corner are held together: |sum - ref sum| within the sum of their bounds"""
    d = _gold(case)
    terms, d_cls, d_reg, keys, loss, tb = _route(_head(CORNER_LOSS_REGULARIZATION=case["corner"]), d, case["B"])
    assert keys == ["rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss"] + (["rcnn_loss_corner"] if case["corner"] else [])
    bd, R = rl.bounds(d)
    assert rl.ratio(d_cls, *bd["d_cls"]) <= 1.0 and rl.ratio(d_reg, *bd["d_reg"]) <= 1.0
    assert abs(tb["rcnn_loss_cls"] - R["out"][0]) <= bd["out_cls"][1][0]
    assert abs(tb["rcnn_loss_reg"] - R["out"][3]) <= bd["out_reg"][1][0] + bd["out_corner"][1][0] + 2.0 ** -23 * abs(R["out"][3])
    if case["corner"]:
        assert abs(tb["rcnn_loss_corner"] - R["out"][2]) <= bd["out_corner"][1][0]


EMULATED = rl.shape_cases() + rl.value_cases() + rl.cap_cases()[:1] + [rl.KITTI_CASE]


def test_emulation_lies_inside_the_bound():
    """the float32 emulation of both launches over the case lists the GPU tests run (poisoned: NaN wherever the labels and the mask exclude)"""
    W = rl.Worst()
    for c in EMULATED:
        d = rl.make_case(c)
        rl.check_roi(W, d, rl.emulate(d), rl.case_name(c))
    for c in CASES:
        d = _gold(c)
        rl.check_roi(W, d, rl.emulate(d), c["name"])
    print(W.report())


def test_value_cases_hold_the_edges_they_name():
    by = {c["kind"]: rl.make_case(c) for c in rl.value_cases() if c["corner"]}
    R = {k: rl.restate(d) for k, d in by.items()}
    assert not R["no_fg"]["fg"].any() and not R["no_valid"]["valid"].any() and R["all_fg"]["fg"].all()
    assert (R["fg_ignored"]["fg"] & ~R["fg_ignored"]["valid"]).any()
    fg = R["dist_zero"]["fg"]
    assert (R["dist_zero"]["m"][fg] == 0).any(), "a prediction equal to its target box"
    m = R["dist_one"]["m"][R["dist_one"]["fg"]]
    assert (m < 1).any() and (m > 1).any() and np.abs(m - 1).min() < 2e-3
    d = by["beta_seam"]
    n = np.abs(d["reg"][:, [2, 6]][d["mask"] > 0])
    assert (n == rl.BETA32).any() and (n == np.nextafter(rl.BETA32, np.float32(1))).any() and (n == np.nextafter(rl.BETA32, np.float32(0))).any()
    tw = rl.restate(by["twin_nearer"])
    assert tw["out"][2] < 2 * rl.restate(by["twin_nearer"], defect="no_twin")["out"][2], "the half-turn twin is the nearer one"
    d = by["tiny_dims"]
    on = d["mask"] > 0
    assert (d["rois"][on][:, 3:6] == 0).any() and ((d["rois"][on][:, 3:6] > 0) & (d["rois"][on][:, 3:6] < 1e-5)).any() and (d["gt"][on][:, 3:6] < 1e-5).any()
    h = by["heading_out"]["rois"][by["heading_out"]["mask"] > 0][:, 6]
    assert (h < 0).any() and (h > 2 * np.pi - 1).any() and rl.margins(by["heading_out"])["trig"] <= 2 * np.pi
    x = by["logit_sat"]["cls"][R["logit_sat"]["valid"]]
    assert {17.0, 20.0, 120.0, -104.0} <= set(x.tolist()) and R["logit_sat"]["sat_hi"].sum() >= 3 and R["logit_sat"]["sat_lo"].any()
    assert np.isnan(by["nan_target"]["gt"][by["nan_target"]["mask"] > 0][:, :7]).any() and not R["nan_target"]["live"][R["nan_target"]["fg"]].all()
    assert by["labels_i64"]["labels"].dtype == np.int64 and (by["labels_i64"]["labels"] == -1).any()


def test_saturated_class_terms_are_exact():
    """one valid roi, so out[0] is the term itself: 100 (1 - t) cls_weight where p rounds to 1.0f, 100 t cls_weight where p underflows; the
    float32 emulation holds the contract bit for bit and its gradient there is exactly 0"""
    for x, t, want in ((17.0, 0.25, 75.0), (20.0, 0.0, 100.0), (120.0, 1.0, 0.0), (120.0, 0.5, 50.0), (-104.0, 0.75, 75.0), (-104.0, 0.0, 0.0)):
        d = rl.make_case(dict(N=1, kind="random", labels="roi_iou", corner=False))
        d["cls"], d["labels"] = np.array([x], np.float32), np.array([t], np.float32)
        for dt in (np.float32, np.float64):
            R = rl.restate(d, dt)
            assert float(R["out"][0]) == want * rl.W_DEFAULT["rcnn_cls_weight"], (x, t, dt)
            assert x < 0 or float(R["d_cls"][0]) == 0.0


@pytest.mark.parametrize("defect", rl.DEFECTS)
def test_the_checks_can_fail(defect):
    """every seeded defect exceeds a bound (or breaks an exact property) on at least one listed case"""
    caught = []
    cases = [(rl.case_name(c), rl.make_case(c)) for c in rl.value_cases() + [rl.KITTI_CASE]] + [(c["name"], _gold(c)) for c in CASES]
    for name, d in cases:
        W = rl.Worst(strict=False)
        rl.check_roi(W, d, rl.emulate(d, defect=defect), name)
        if max(W.worst.values()) > 1.0:
            caught.append((name, {k: v for k, v in W.worst.items() if v > 1.0}))
    print(defect, "caught on %d of %d cases, e.g." % (len(caught), len(cases)), caught[:2])
    assert caught, defect


def test_poison_changes_nothing_in_the_restatement():
    for c in rl.value_cases()[:6] + [rl.KITTI_CASE]:
        a, b = rl.restate(rl.make_case(c, poison=True)), rl.restate(rl.make_case(c, poison=False))
        for k in ("out", "d_cls", "d_reg"):
            assert np.array_equal(a[k], b[k]), (c, k)


# ------------------------------------------------------------------------------------------------------------------------- the module
def test_unsupported_reason_names_the_bar():
    from btcdet_amd import roi_loss
    from btcdet_amd.dense_head import ResidualCoder
    cfg = _head().model_cfg.LOSS_CONFIG
    assert roi_loss.unsupported_reason(cfg, ResidualCoder()) is None
    assert "CLS_LOSS" in roi_loss.unsupported_reason(dict(cfg, CLS_LOSS="CrossEntropy"), ResidualCoder())
    assert "REG_LOSS" in roi_loss.unsupported_reason(dict(cfg, REG_LOSS="l1"), ResidualCoder())
    assert "encode_angle_by_sincos" in roi_loss.unsupported_reason(cfg, ResidualCoder(encode_angle_by_sincos=True))
    assert "code size of 9" in roi_loss.unsupported_reason(cfg, ResidualCoder(code_size=9))
    with pytest.raises(ValueError, match="no CPU fallback"):
        roi_loss.roi_loss(_fill(_head(), _gold(CASES[0]), CASES[0]["B"]), rl.W_DEFAULT)
    assert (roi_loss.THREADS, roi_loss.LANES, roi_loss.MAX_TILES) == (rl.THREADS, rl.LANES, rl.MAX_TILES)


def test_cpu_tensors_keep_the_torch_route_and_the_key_is_opt_in(caplog):
    case = CASES[0]
    d = _gold(case)
    plain, keyed, off = _head(), _head(True), _head(False)
    res = [_route(h, d, case["B"]) for h in (plain, keyed, off)]
    assert keyed.device_loss and not plain.device_loss and not off.device_loss
    assert res[0][5] == res[1][5] and res[0][4] == res[1][4], "CPU tensors: the keyed head gives the bits of the torch route"
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    assert res[0][3] == ["rcnn_loss_cls", "rcnn_loss_reg", "rcnn_loss", "rcnn_loss_corner"]
    # an unsupported configuration keeps the torch route and says why, once
    bad = _head(True, CLS_LOSS="CrossEntropy")
    _fill(bad, d, case["B"])
    bad.forward_ret_dict["rcnn_cls_labels"] = torch.zeros_like(bad.forward_ret_dict["rcnn_cls_labels"], dtype=torch.int64)   # one class: index 0
    with caplog.at_level(logging.WARNING, logger="btcdet_amd.conv_head"):
        bad.get_loss()
        bad.get_loss()
    said = [r.getMessage() for r in caplog.records if "LOSS_CONFIG.DEVICE" in r.getMessage()]
    assert not bad.device_loss and len(said) == 1 and "CLS_LOSS" in said[0] and "torch route" in said[0]
    for name in ("btcdet_kitti_car.yaml", "btcdet_waymo_synth.yaml"):
        assert "DEVICE" not in open(os.path.join(ROOT, "btcdet_amd", "cfgs", name)).read(), "the shipped configurations stay without the key"


# ------------------------------------------------------------------------------------------------------------------------- C ABI
def test_ctypes_table_matches_the_header():
    from btcdet_amd import _lib
    src = open(os.path.join(ROOT, "include", "btcdet_hip_roi_loss.h")).read()
    for line in ("e = expf(-|x|) ; r = 1 / (1 + e) ; p = x >= 0 ? r : e * r ; om = 1 - p", "term = (t - 1) * max(logf(om), -100) - t * max(logf(p), -100)",
                 "d = r_k - v_k ; n = |d| ; term = n < beta ? 0.5 * (n * n) / beta : n - 0.5 * beta",
                 "D = P - Q ; dist(Q) = sqrtf((D_x * D_x + D_y * D_y) + D_z * D_z) ; m = min(dist(Q), dist(Q'))",
                 "out[3]      = out[1] + out[2] ; out[4] = out[0] + out[3], both in float32", "the UNFLIPPED twin takes the whole gradient"):
        assert line in src, "the header states its formulas: " + line
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.ROI_LOSS_EXPORTED_SYMBOLS) == ["btc_roi_loss_bwd", "btc_roi_loss_fwd", "btc_roi_loss_ws_bytes"]
    L = _lib.lib()
    kinds = {"int": _lib.ci, "size_t": _lib.sz, "float": _lib.cf}
    for n, count in (("btc_roi_loss_fwd", 19), ("btc_roi_loss_bwd", 19), ("btc_roi_loss_ws_bytes", 1)):
        assert hasattr(L, n)
        res, args = _lib._ROI_LOSS_SIGS[n]
        m = re.search(r"(size_t|int)\s+%s\s*\(([^)]*)\)" % n, src)
        assert kinds[m.group(1)] is res, n
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args) == count, n
        for p, a in zip(params, args):
            want = _lib.vp if "*" in p else kinds[re.sub(r"\s+\w+$", "", p).replace("const ", "").strip()]
            assert a is want, (n, p)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "btcdet_hip_roi_loss.h":
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
            assert not set(names) & set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", text)), other
    assert rl.TILE * rl.LANES == rl.THREADS and rl.LANES in (1, 8)
    ws = L.btc_roi_loss_ws_bytes
    assert ws(-1) == 0 and ws(2 ** 28) == 0 and ws(2 ** 28 - 1) == 256 + rl.MAX_TILES * 40
    assert ws(0) == ws(1) == ws(rl.TILE) == 256 + 40 and ws(rl.TILE + 1) == 256 + 2 * 40
    assert ws(rl.CAP) == ws(rl.CAP + 1) == 256 + rl.MAX_TILES * 40


def test_refusals_need_no_device():
    """every refusal happens before any launch, so it can be asked for without a GPU; the device pointers are never read"""
    from btcdet_amd import _lib
    L = _lib.lib()
    fake = 1 << 20
    N = 300
    ws_bytes = L.btc_roi_loss_ws_bytes(N)
    fwd = dict(cls=fake, reg=fake, rois=fake, gt=fake, src=fake, gt_width=8, mask=fake, labels=fake, kind=0, N=N, corner=1, cw=1.0, rw=1.0, kw=1.0,
               out=fake, norms=fake, ws=fake, ws_bytes=ws_bytes)
    bwd = dict(list(fwd.items())[:14], norms=fake, grad=fake, d_cls=fake, d_reg=fake)
    common = [dict(N=-1), dict(N=2 ** 28), dict(gt_width=6), dict(kind=2), dict(kind=-1), dict(cls=None), dict(reg=None), dict(rois=None), dict(gt=None),
              dict(src=None), dict(mask=None), dict(labels=None)]
    for fn, good, extra in ((L.btc_roi_loss_fwd, fwd, [dict(out=None), dict(norms=None), dict(ws=None), dict(ws_bytes=ws_bytes - 1), dict(ws_bytes=0)]),
                            (L.btc_roi_loss_bwd, bwd, [dict(norms=None), dict(grad=None), dict(d_cls=None), dict(d_reg=None)])):
        for kw in common + extra:
            a = dict(good, **kw)
            assert fn(*a.values(), None) == -1, kw
            assert L.btc_last_error().decode().startswith("btc_roi_loss_"), kw
    # legal and launching nothing: the backward over no rois
    none = dict(cls=None, reg=None, rois=None, gt=None, src=None, mask=None, labels=None, d_cls=None, d_reg=None)
    assert L.btc_roi_loss_bwd(*dict(bwd, N=0, **none).values(), None) == 0
