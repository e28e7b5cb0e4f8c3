"""btc_roi_targets (csrc/roi_targets.hip, include/btcdet_hip_roi_targets.h) through btcdet_amd.roi_targets_device on the GPU: against the numpy
restatement of the header (tests/roi_targets_ref.py: bit for bit, the two rotated columns inside the derived bound; the BEV overlaps from
btc_boxes_pairwise_bev mode 0 on the same boxes), against the torch route on the same uniforms (every key of its dict), against the
reference's own record with its own draw handed over, and its behaviour: identical bits on identical calls, a workspace that needs no
clearing, ConvHead with TARGET_CONFIG.DEVICE, and no touch of the symbol with the flag unset."""
import copy
import os

import numpy as np
import pytest
import torch

import roi_targets_ref as rr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KEYS = ("rois", "roi_scores", "roi_labels", "gt_boxes")


def _batch(case):
    bd = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(DEV) for k in KEYS}
    bd["batch_size"] = case["batch_size"]
    return bd


def _bev(case):
    """(B, N, G): btc_boxes_pairwise_bev mode 0 on the case's boxes"""
    from btcdet_amd.iou3d_nms import _pairwise
    B = case["batch_size"]
    return np.stack([_pairwise(torch.from_numpy(case["rois"][b]).to(DEV), torch.from_numpy(np.ascontiguousarray(case["gt_boxes"][b][:, :7])).to(DEV), 0).cpu().numpy()
                     for b in range(B)])


def _np(t):
    return {k: v.cpu().numpy() for k, v in t.items()}


@pytest.fixture(scope="module")
def runs():
    """every listed case once: the inputs, the device route's outputs, the BEV overlaps and both restatements -- shared and left unchanged"""
    from btcdet_amd.roi_targets_device import DeviceProposalTargets
    out = {}
    for spec in rr.CASES:
        case = rr.make_case(spec)
        bd = _batch(case)
        u = torch.from_numpy(case["uniforms"]).to(DEV)
        got = _np(DeviceProposalTargets(case["cfg"])(bd, uniforms=u))
        bev = _bev(case)
        out[spec["name"]] = dict(case=case, bd=bd, u=u, got=got, bev=bev, emu=rr.restate(case, bev, np.float32), ref=rr.restate(case, bev, np.float64))
    return out


@pytest.mark.parametrize("name", rr.CASE_IDS)
def test_against_the_restatement(runs, name):
    r = runs[name]
    case, got = r["case"], r["got"]
    m = rr.margins(got["max_overlaps"], got["gt_iou_of_rois"], case["uniforms"], case["cfg"])
    assert rr.clear(m) and rr.foreground_keys_distinct(got["max_overlaps"], case["uniforms"], case["cfg"]), m
    # the closed-form overlaps of the case list and the kernel's agree on every candidate set
    ana = rr.restate(case, rr.analytic_bev(case), np.float32)
    # (hard and easy rois to 2e-4; a foreground roi nearly coincides with its box, where box_overlap -- the reference's formulation -- counts
    # corners up to its 1e-2 margin outside as inside: the polygon may grow by margin x perimeter at either rectangle, 4 x 0.01 x 11 m of 6.2 m2)
    c = rr.consts(case["cfg"])
    fg = ana["max_overlaps"] >= c.fg_thresh
    assert np.array_equal(got["max_overlaps"] >= c.fg_thresh, fg) and np.array_equal(got["max_overlaps"] < c.cls_bg_lo, ana["max_overlaps"] < c.cls_bg_lo)
    np.testing.assert_allclose(got["max_overlaps"][~fg], ana["max_overlaps"][~fg], rtol=0, atol=2e-4)
    np.testing.assert_allclose(got["max_overlaps"][fg], ana["max_overlaps"][fg], rtol=0, atol=0.08)
    assert np.array_equal(got["sampled_inds"], ana["sampled_inds"]) and np.array_equal(got["gt_assignment"], ana["gt_assignment"])
    worst = rr.check_outputs(got, r["emu"], r["ref"], name)
    print(name, "margins", m, "rotated columns: worst err / bound %.3f" % worst)
    R = int(case["cfg"].ROI_PER_IMAGE)
    want_cls = np.float32 if case["cfg"].CLS_SCORE_TYPE == "roi_iou" else np.int64
    assert got["rcnn_cls_labels"].dtype == want_cls and got["reg_valid_mask"].dtype == np.int64 and got["sampled_inds"].shape == (case["batch_size"], R)


@pytest.mark.parametrize("name", rr.CASE_IDS)
def test_against_the_torch_route_on_the_same_uniforms(runs, name):
    from btcdet_amd.roi_targets import ProposalTargetLayer, canonical_targets, match_rois
    from btcdet_amd import iou3d_nms
    r = runs[name]
    case, got, cfg = r["case"], r["got"], r["case"]["cfg"]
    t = _np(canonical_targets(ProposalTargetLayer(cfg)(r["bd"], uniforms=r["u"])))
    assert set(t) <= set(got) and set(got) - set(t) == {"max_overlaps", "gt_assignment", "sampled_inds"}
    for k, v in t.items():
        assert v.dtype == got[k].dtype and v.shape == got[k].shape, k
    keys = tuple(k for k in t if k != "gt_of_rois")
    # exact where the restatement is exact -- the torch route's bits -- and the bound elsewhere
    rr.check_outputs(t, r["emu"], r["ref"], name + " (torch route)", keys=keys + ("gt_of_rois",))
    for k in keys:
        assert rr.same_bits(t[k], got[k]), k
    assert rr.same_bits(t["gt_of_rois"][..., 2:], got["gt_of_rois"][..., 2:])
    bound = rr.rotated_bound(got["rois"], got["gt_of_rois_src"])
    assert (np.abs(t["gt_of_rois"][..., :2].astype(np.float64) - got["gt_of_rois"][..., :2]) <= 2 * bound).all()
    print(name, "rotated columns equal the torch route's bits:", rr.same_bits(t["gt_of_rois"], got["gt_of_rois"]))
    for b in range(case["batch_size"]):
        if cfg.SAMPLE_ROI_BY_EACH_CLASS:
            ov, arg = match_rois(r["bd"]["rois"][b], r["bd"]["roi_labels"][b], r["bd"]["gt_boxes"][b])
        else:
            ov, arg = iou3d_nms.boxes_iou3d_gpu(r["bd"]["rois"][b], r["bd"]["gt_boxes"][b][:, 0:7].contiguous()).max(dim=1)
        assert rr.same_bits(ov.cpu().numpy(), got["max_overlaps"][b]) and np.array_equal(arg.cpu().numpy(), got["gt_assignment"][b]), b


def _golden():
    import common
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_targets.npz"))
    inp = common.roi_target_inputs()
    case = dict(inp, cfg=rr.make_cfg())
    return g, case


def test_against_the_reference_record_with_its_own_draw():
    """the assertions of test_hip_roi_targets.py::test_matching_targets_and_canonical_transform_vs_reference, on the device route"""
    from btcdet_amd.config import load_cfg
    from btcdet_amd.roi_targets_device import DeviceProposalTargets
    g, case = _golden()
    cfg = load_cfg().MODEL.ROI_HEAD
    sel = torch.from_numpy(g["sampled_inds"]).to(DEV)
    t = _np(DeviceProposalTargets(cfg.TARGET_CONFIG)(_batch(case), sampled_inds=sel))
    np.testing.assert_allclose(t["max_overlaps"], g["max_overlaps"], rtol=0, atol=2e-5)
    assert np.array_equal(t["sampled_inds"], g["sampled_inds"])
    for k in ("rois", "roi_scores", "gt_of_rois_src"):
        assert np.array_equal(t[k], g["t_" + k]), k
    assert np.array_equal(t["roi_labels"], g["t_roi_labels"])
    np.testing.assert_allclose(t["gt_iou_of_rois"], g["t_gt_iou_of_rois"], rtol=0, atol=2e-5)
    iou = g["t_gt_iou_of_rois"]
    clear = np.ones_like(iou, bool)
    for th in (cfg.TARGET_CONFIG.REG_FG_THRESH, cfg.TARGET_CONFIG.CLS_FG_THRESH, cfg.TARGET_CONFIG.CLS_BG_THRESH):
        clear &= np.abs(iou - th) > 1e-4
    assert clear.mean() > 0.99
    assert np.array_equal(t["reg_valid_mask"][clear], g["t_reg_valid_mask"][clear])
    np.testing.assert_allclose(t["rcnn_cls_labels"][clear], g["t_rcnn_cls_labels"][clear], rtol=0, atol=1e-4)
    np.testing.assert_allclose(t["gt_of_rois"], g["t_gt_of_rois"], rtol=0, atol=2e-5)
    # and the restatement on the same realistic proposals (jittered boxes: overlaps of every size), the draw handed over and sampled
    bev = _bev(case)
    rr.check_outputs(t, rr.restate(case, bev, np.float32, sampled_in=g["sampled_inds"]), rr.restate(case, bev, np.float64, sampled_in=g["sampled_inds"]), "golden")
    import common
    case["uniforms"] = common._hash01(3 * 4 * 512, 77).reshape(3, 4, 512)
    assert rr.foreground_keys_distinct(t["max_overlaps"], case["uniforms"], case["cfg"])
    own = _np(DeviceProposalTargets(cfg.TARGET_CONFIG)(_batch(case), uniforms=torch.from_numpy(case["uniforms"]).to(DEV)))
    rr.check_outputs(own, rr.restate(case, bev, np.float32), rr.restate(case, bev, np.float64), "golden, sampled")


def test_identical_calls_give_identical_bits_and_the_workspace_needs_no_clearing(runs):
    from btcdet_amd import roi_targets_device as rtd
    r = runs["n512_cls"]
    layer = rtd.DeviceProposalTargets(r["case"]["cfg"])
    for _ in range(2):                                              # the same cached workspace, never cleared between the calls
        again = _np(layer(r["bd"], uniforms=r["u"]))
        for k, v in r["got"].items():
            assert rr.same_bits(again[k], v), k
    ws = [w for (dev, _), w in rtd._WS.items() if dev == DEV.index]
    assert ws and all(not bool(w.any()) for w in ws), "the counters are left zero"
    # its own draw: one rand per batch, fresh on every call, the same stream for the same seed
    a, b = rtd.DeviceProposalTargets(r["case"]["cfg"], seed=5), rtd.DeviceProposalTargets(r["case"]["cfg"], seed=5)
    a1, a2, b1 = a(r["bd"])["sampled_inds"], a(r["bd"])["sampled_inds"], b(r["bd"])["sampled_inds"]
    assert torch.equal(a1, b1) and not torch.equal(a1, a2)


def _head(device_flag):
    from btcdet_amd.btc_path import BtcHotPath
    from btcdet_amd.config import load_cfg
    cfg = copy.deepcopy(load_cfg())
    if device_flag:
        cfg.MODEL.ROI_HEAD.TARGET_CONFIG["DEVICE"] = True
    torch.manual_seed(0)
    return BtcHotPath(cfg, device=DEV, heads="full").to(DEV).train()


def test_conv_head_with_the_device_flag_trains(monkeypatch):
    """one --heads full-shaped forward, loss and backward with TARGET_CONFIG.DEVICE: finite, every ROI-head parameter gets a gradient, and
    the targets came from btc_roi_targets"""
    import bench
    from btcdet_amd import roi_targets_device as rtd
    calls = []
    orig = rtd.DeviceProposalTargets.forward
    monkeypatch.setattr(rtd.DeviceProposalTargets, "forward", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    model = _head(True)
    batches = bench.build_batches(2, 0, DEV)
    out, tb, bd = model(model.prepare(batches[0]))
    loss = model.det_loss(out, bd) + out["loss_occ"]
    loss.backward()
    assert torch.isfinite(loss) and calls
    missing = [n for n, p in model.det_modules.roi_head.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not missing, missing
    ret = model.det_modules.roi_head.forward_ret_dict
    assert {"max_overlaps", "gt_assignment", "sampled_inds"} <= set(ret) and ret["rcnn_cls_labels"].dtype == torch.float32


def test_without_the_flag_the_symbol_is_not_touched(monkeypatch):
    from btcdet_amd import roi_targets_device as rtd
    from btcdet_amd.config import load_cfg
    from btcdet_amd.conv_head import ConvHead

    def boom(*a, **k):
        raise AssertionError("the device route was taken without TARGET_CONFIG.DEVICE")
    monkeypatch.setattr(rtd.DeviceProposalTargets, "forward", boom)
    monkeypatch.setattr(rtd.DeviceProposalTargets, "__init__", boom)
    g, case = _golden()
    cfg = load_cfg()
    assert "DEVICE" not in cfg.MODEL.ROI_HEAD.TARGET_CONFIG
    head = ConvHead.__new__(ConvHead)
    torch.nn.Module.__init__(head)
    head.model_cfg = cfg.MODEL.ROI_HEAD
    t = head.assign_targets(_batch(case), torch.from_numpy(g["sampled_inds"]).to(DEV))
    assert head.device_targets is False and "max_overlaps" not in t and np.array_equal(t["rois"].cpu().numpy(), g["t_rois"])
    # with the flag the same head object takes the device route and returns the same deterministic targets
    monkeypatch.undo()
    cfg2 = copy.deepcopy(cfg)
    cfg2.MODEL.ROI_HEAD.TARGET_CONFIG["DEVICE"] = True
    head2 = ConvHead.__new__(ConvHead)
    torch.nn.Module.__init__(head2)
    head2.model_cfg = cfg2.MODEL.ROI_HEAD
    t2 = head2.assign_targets(_batch(case), torch.from_numpy(g["sampled_inds"]).to(DEV))
    assert "max_overlaps" in t2
    for k in t:
        if k != "gt_of_rois":
            assert torch.equal(t[k], t2[k]), k
    assert torch.allclose(t["gt_of_rois"], t2["gt_of_rois"], rtol=0, atol=2e-5)
