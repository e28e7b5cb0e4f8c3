"""btc_anchor_targets and btc_decode_anchor_boxes (csrc/anchor_targets.hip, include/btcdet_hip_heads.h) through
btcdet_amd.anchor_targets: against the reference's own outputs (tests/golden/anchor_targets.npz and head.npz at KITTI size), against the
torch formulation (dense_head.AxisAlignedTargetAssigner) on the same device and the numpy restatement at the kernel's shape edges,
without a synchronisation, and wired into AnchorHeadSingle.

Labels, weights and the columns without a transcendental (0, 1, 2, 6) are exact; the log / exp columns at rtol 1e-5, atol 1e-6 (the
tolerance tests/test_hip_dense_head.py gives those values: logf / expf of the device library against the host's)."""
import numpy as np
import pytest
import torch

import anchor_targets_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXACT = list(ar.EXACT)
G, CASES = ar.gold()


def _coder():
    from btcdet_amd.dense_head import ResidualCoder
    return ResidualCoder()


def _anchors(map_name, cfg):
    from btcdet_amd.dense_head import make_anchors
    m = ar.MAPS[map_name]
    return make_anchors(np.array(m["point_cloud_range"], np.float32), cfg.ANCHOR_GENERATOR_CONFIG, np.array(m["grid_size"]), DEV)[0]


def _np(d):
    return d["box_cls_labels"].cpu().numpy(), d["box_reg_targets"].cpu().numpy(), d["reg_weights"].cpu().numpy()


def _report(what, got, want):
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("%s: max |diff| exact columns %.3e, log/exp columns %.3e" % (what, diff[..., EXACT].max(initial=0), diff[..., list(ar.TRANSCENDENTAL)].max(initial=0)))


# ------------------------------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] == "assign"], ids=lambda c: c["name"])
def test_assignment_equals_the_reference(case):
    from btcdet_amd.anchor_targets import DeviceTargetAssigner
    name, mp = case["name"], case["map"]
    cfg = ar.head_cfg(mp, case["matched"], case["unmatched"])
    assigner = DeviceTargetAssigner(cfg, ar.MAPS[mp]["class_names"], _coder())
    labels, targets, weights = _np(assigner.assign_targets(_anchors(mp, cfg), torch.from_numpy(G[name + "/gt"]).to(DEV)))
    _report(name, targets, G[name + "/targets"])
    print("labels differing", int((labels != G[name + "/labels"]).sum()), "positives", int((labels > 0).sum()))
    assert labels.dtype == np.int32 and np.array_equal(labels, G[name + "/labels"].astype(np.int32))
    assert np.array_equal(weights, G[name + "/weights"])
    assert np.array_equal(targets[..., EXACT], G[name + "/targets"][..., EXACT])
    np.testing.assert_allclose(targets, G[name + "/targets"], rtol=1e-5, atol=1e-6)


def test_assignment_equals_head_npz_at_kitti_size():
    from btcdet_amd.anchor_targets import DeviceTargetAssigner
    cfg, names, anchors, g = ar.kitti_head()
    assigner = DeviceTargetAssigner(cfg, names, _coder())
    out = assigner.assign_targets([a.to(DEV) for a in anchors], torch.from_numpy(g["gt_boxes"]).to(DEV))
    labels, targets, weights = _np(out)
    assert labels.shape == (2, 70400)
    print("positives", int((labels > 0).sum()), "ignored", int((labels < 0).sum()))
    ar.check_against_head_npz(labels, targets, weights, g)


@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] == "decode"], ids=lambda c: c["name"])
def test_decode_equals_the_reference(case):
    from btcdet_amd.anchor_targets import decode_boxes
    name, cfg = case["name"], ar.head_cfg(case["map"])
    dirs = torch.from_numpy(G[name + "/dir_cls_preds"]).to(DEV) if case["dir"] else None
    preds = torch.from_numpy(G[name + "/box_preds"]).to(DEV).requires_grad_(True)
    boxes = decode_boxes(preds, torch.from_numpy(G["anchors/" + case["map"]]).to(DEV), dirs, cfg)
    assert not boxes.requires_grad
    boxes = boxes.cpu().numpy()
    _report(name, boxes, G[name + "/boxes"])
    assert np.array_equal(boxes[..., EXACT], G[name + "/boxes"][..., EXACT])
    np.testing.assert_allclose(boxes, G[name + "/boxes"], rtol=1e-5, atol=1e-6)


# -------------------------------------------------------------------------------------------------------------------- shape edges
RANGE = [0.0, -12.0, -3.0, 24.0, 12.0, 1.0]
ONE_SLOT = [dict(class_name="Car", anchor_sizes=[[3.9, 1.6, 1.56]], anchor_rotations=[0], anchor_bottom_heights=[-1.78], align_center=True,
                 feature_map_stride=1, matched_threshold=0.6, unmatched_threshold=0.45)]
TWO_SLOTS = [dict(ONE_SLOT[0], anchor_rotations=[0, 1.57])]
THREE_CFGS = [dict(g, align_center=True, feature_map_stride=1) for g in ar.MAPS["three"]["generator"]]
# (nx, ny, generator, class names) -> A = ny * nx * slots; 256 threads per workgroup, a workgroup inside one scene
GRIDS = {"A0": (17, 15, ONE_SLOT, ["Car"]), "A1": (1, 1, ONE_SLOT, ["Car"]), "A255": (17, 15, ONE_SLOT, ["Car"]), "A256": (16, 16, ONE_SLOT, ["Car"]),
         "A257": (1, 257, ONE_SLOT, ["Car"]), "A513": (27, 19, ONE_SLOT, ["Car"]), "A510": (17, 15, TWO_SLOTS, ["Car"]),
         "A512": (16, 16, TWO_SLOTS, ["Car"]), "A514": (1, 257, TWO_SLOTS, ["Car"]), "A1530": (17, 15, THREE_CFGS, ar.MAPS["three"]["class_names"])}
_EDGE = {}


def edge_case(grid, M):
    """-> (cfg, class names, anchors on the device, gt (3, M, 8)): scene 0 has M boxes, scene 1 fewer with a padded tail, scene 2 one box;
    the first seed whose boxes pass the generator's margin check; made once per (grid, M)"""
    from btcdet_amd.dense_head import make_anchors
    if (grid, M) not in _EDGE:
        nx, ny, gen, names = GRIDS[grid]
        cfg = ar.head_cfg("one")
        cfg.ANCHOR_GENERATOR_CONFIG = [ar.ED(g) for g in gen]
        anchors = make_anchors(np.array(RANGE, np.float32), cfg.ANCHOR_GENERATOR_CONFIG, np.array([nx, ny, 40]), "cpu")[0]
        if grid == "A0":
            anchors = [a[:, :0].contiguous() for a in anchors]
        flat = torch.cat(anchors, dim=-3).reshape(-1, 7).numpy()
        assert flat.shape[0] == int(grid[1:])
        tables = ar.host_tables(cfg, names)
        for seed in range(100):
            rng = np.random.default_rng(977 * M + seed)
            gt = np.zeros((3, M, 8), np.float32)
            if M:
                gt[0] = ar.random_boxes(rng, M, len(names), (1, -11, 23, 11))
                gt[1] = ar.random_boxes(rng, M // 2, len(names), (1, -11, 23, 11), pad=M - M // 2)
                gt[2] = ar.random_boxes(rng, 1, len(names), (1, -11, 23, 11), pad=M - 1)
            try:
                want = ar.margins_assign(flat, *tables, gt)
                break
            except AssertionError:
                continue
        else:
            raise AssertionError("no seed passes the margins")
        _EDGE[(grid, M)] = (cfg, names, [a.to(DEV) for a in anchors], gt, want)
    return _EDGE[(grid, M)]


@pytest.mark.parametrize("M", [0, 1, 64, 65])
@pytest.mark.parametrize("grid", sorted(GRIDS, key=lambda g: int(g[1:])))
def test_shape_edges_equal_the_torch_route_and_the_restatement(grid, M):
    from btcdet_amd.anchor_targets import DeviceTargetAssigner
    from btcdet_amd.dense_head import AxisAlignedTargetAssigner
    cfg, names, anchors, gt, want = edge_case(grid, M)
    d_gt = torch.from_numpy(gt).to(DEV)
    labels, targets, weights = _np(DeviceTargetAssigner(cfg, names, _coder()).assign_targets(anchors, d_gt))
    r_labels, r_targets, r_weights, r_best = want[:4]
    if grid == "A0":                                                  # the torch route cannot shape an empty grid: the restatement alone
        t_labels, t_targets, t_weights = r_labels, r_targets, r_weights
    else:
        t_labels, t_targets, t_weights = _np(AxisAlignedTargetAssigner(cfg, names, _coder()).assign_targets(anchors, d_gt.clone()))
    _report("%s M %d against the restatement" % (grid, M), targets, r_targets)
    _report("%s M %d against the torch route" % (grid, M), targets, t_targets)
    print("positives", int((labels > 0).sum()), "ignored", int((labels < 0).sum()), "of", labels.size)
    assert np.array_equal(labels, r_labels) and np.array_equal(labels, t_labels)
    assert np.array_equal(weights, r_weights) and np.array_equal(weights, t_weights)
    # the matched box: the columns without a transcendental are a function of (anchor, matched box) alone, and the boxes are distinct
    assert np.array_equal(targets[..., EXACT], r_targets[..., EXACT])
    np.testing.assert_allclose(targets, r_targets, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(targets, t_targets, rtol=1e-5, atol=1e-6)
    assert np.array_equal(targets[..., 6], t_targets[..., 6]), "the matched box's heading, a plain difference on both routes"
    print("anchors whose matched box lies in the second staged chunk:", int((r_best >= 64).sum()))


# -------------------------------------------------------------------------------------------------------------- no synchronisation
def test_the_fused_route_synchronises_nowhere():
    from btcdet_amd.dense_head import AnchorHeadSingle
    m = ar.MAPS["one"]
    head = AnchorHeadSingle(ar.head_cfg("one", device=True), input_channels=8, num_class=1, class_names=m["class_names"], grid_size=np.array(m["grid_size"]),
                            point_cloud_range=np.array(m["point_cloud_range"], np.float32)).to(DEV)
    gt = torch.from_numpy(G["one_mixed/gt"]).to(DEV)
    cls = torch.randn(3, 16, 16, 2, device=DEV)
    box = torch.randn(3, 16, 16, 14, device=DEV)
    dirs = torch.randn(3, 16, 16, 4, device=DEV)
    anchors = head.anchors(torch.device(DEV))
    first = head.target_assigner.assign_targets(anchors, gt)            # loads the library, builds the anchors
    head.generate_predicted_boxes(3, cls, box, dirs)
    probe = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.sum().item()
            raised = False
        except RuntimeError:
            raised = True
        if not raised:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag .item() on this build: the mode cannot show the absence of a read-back")
        again = head.target_assigner.assign_targets(anchors, gt)
        _, boxes = head.generate_predicted_boxes(3, cls, box, dirs)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert boxes.shape == (3, 512, 7)
    for k in first:
        assert torch.equal(first[k], again[k])
    assert np.array_equal(again["box_cls_labels"].cpu().numpy(), G["one_mixed/labels"].astype(np.int32))


# --------------------------------------------------------------------------------------------------------------------- head wiring
def test_head_with_the_device_route_equals_the_head_without():
    from btcdet_amd.anchor_targets import DeviceTargetAssigner
    from btcdet_amd.dense_head import AnchorHeadSingle, AxisAlignedTargetAssigner
    m = ar.MAPS["one"]

    def head(cfg):
        torch.manual_seed(3)
        return AnchorHeadSingle(cfg, input_channels=8, num_class=1, class_names=m["class_names"], grid_size=np.array(m["grid_size"]),
                                point_cloud_range=np.array(m["point_cloud_range"], np.float32)).to(DEV).train()
    off, on = head(ar.head_cfg("one")), head(ar.head_cfg("one", device=True))
    assert type(off.target_assigner) is AxisAlignedTargetAssigner and type(on.target_assigner) is DeviceTargetAssigner
    torch.manual_seed(4)
    x = torch.randn(3, 8, 16, 16, device=DEV)
    gt = torch.from_numpy(G["one_mixed/gt"]).to(DEV)
    res = []
    for h in (off, on):
        d = h({"spatial_features_2d": x, "gt_boxes": gt.clone(), "batch_size": 3})
        labels = h.forward_ret_dict["box_cls_labels"].clone()
        loss, _ = h.get_loss()
        res.append((labels, loss.detach(), d["batch_box_preds"], d["batch_cls_preds"]))
    print("rpn loss off %.9g on %.9g" % (float(res[0][1]), float(res[1][1])))
    assert torch.equal(res[0][0], res[1][0]) and int((res[0][0] > 0).sum()) > 0
    torch.testing.assert_close(res[1][1], res[0][1], rtol=1e-6, atol=0)
    assert torch.equal(res[0][3], res[1][3])
    assert not res[1][2].requires_grad
    torch.testing.assert_close(res[1][2], res[0][2].detach(), rtol=1e-5, atol=1e-6)
    on.zero_grad()
    d = on({"spatial_features_2d": x, "gt_boxes": gt.clone(), "batch_size": 3})
    on.get_loss()[0].backward()                                        # the loss still reaches the head's parameters
    assert on.conv_box.weight.grad is not None and float(on.conv_box.weight.grad.abs().sum()) > 0
