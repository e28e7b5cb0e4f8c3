"""btcdet_amd/anchor_targets.py without a GPU: the numpy restatement of include/btcdet_hip_heads.h (anchor_targets_ref.restate_assign /
restate_decode) against the reference's own outputs (tests/golden/anchor_targets.npz, made by gen_anchor_targets_golden.py; and the
labels, target rows and target values of head.npz at KITTI size), DeviceTargetAssigner.supported and its refusals, the host tables, the
ctypes table against the header and the refusals that need no launch.

Labels, weights, target columns 0, 1, 2, 6 and box columns 0, 1, 2, 6 are exact; the log / exp columns at rtol 1e-5, atol 1e-6 (what
tests/test_hip_dense_head.py gives those values)."""
import os
import re

import numpy as np
import pytest
import torch

import anchor_targets_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = list(ar.EXACT)
G, CASES = ar.gold()


def _anchors(map_name, cfg=None):
    from btcdet_amd.dense_head import make_anchors
    m = ar.MAPS[map_name]
    cfg = cfg or ar.head_cfg(map_name)
    return make_anchors(np.array(m["point_cloud_range"], np.float32), cfg.ANCHOR_GENERATOR_CONFIG, np.array(m["grid_size"]), "cpu")[0]


@pytest.mark.parametrize("map_name", sorted(ar.MAPS))
def test_anchors_equal_the_reference(map_name):
    flat = torch.cat(_anchors(map_name), dim=-3).reshape(-1, 7).numpy()
    assert np.array_equal(flat, G["anchors/" + map_name])


@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] == "assign"], ids=lambda c: c["name"])
@pytest.mark.parametrize("recip", [True, False], ids=["reciprocal", "division"])
def test_restatement_equals_the_reference_assignment(case, recip):
    name = case["name"]
    cfg = ar.head_cfg(case["map"], case["matched"], case["unmatched"])
    tables = ar.host_tables(cfg, ar.MAPS[case["map"]]["class_names"])
    gt = G[name + "/gt"]
    ar.margins_assign(G["anchors/" + case["map"]], *tables, gt, on_edge=case["on_edge"])
    labels, targets, weights, _ = ar.restate_assign(G["anchors/" + case["map"]], *tables, gt, recip=recip)
    assert np.array_equal(labels, G[name + "/labels"].astype(np.int32))
    assert np.array_equal(weights, G[name + "/weights"])
    assert np.array_equal(targets[..., EXACT], G[name + "/targets"][..., EXACT])
    np.testing.assert_allclose(targets, G[name + "/targets"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", [c for c in CASES if c["kind"] == "decode"], ids=lambda c: c["name"])
@pytest.mark.parametrize("recip", [True, False], ids=["reciprocal", "division"])
def test_restatement_equals_the_reference_decode(case, recip):
    name, cfg = case["name"], ar.head_cfg(case["map"])
    dirs = G[name + "/dir_cls_preds"] if case["dir"] else None
    ar.margins_decode(G[name + "/box_preds"], G["anchors/" + case["map"]], dirs, cfg.DIR_OFFSET, cfg.DIR_LIMIT_OFFSET, cfg.NUM_DIR_BINS)
    boxes = ar.restate_decode(G[name + "/box_preds"], G["anchors/" + case["map"]], dirs, cfg.DIR_OFFSET, cfg.DIR_LIMIT_OFFSET, cfg.NUM_DIR_BINS, recip)
    assert np.array_equal(boxes[..., EXACT], G[name + "/boxes"][..., EXACT])
    np.testing.assert_allclose(boxes, G[name + "/boxes"], rtol=1e-5, atol=1e-6)


def test_restatement_equals_head_npz_at_kitti_size():
    cfg, names, anchors, g = ar.kitti_head()
    flat = torch.cat(anchors, dim=-3).reshape(-1, 7).numpy()
    assert flat.shape == (70400, 7)
    labels, targets, weights, _ = ar.restate_assign(flat, *ar.host_tables(cfg, names), g["gt_boxes"])
    ar.check_against_head_npz(labels, targets, weights, g)


# ------------------------------------------------------------------------------------------------------------------- the module
def test_supported_and_refusals():
    from btcdet_amd.anchor_targets import DeviceTargetAssigner
    from btcdet_amd.dense_head import ResidualCoder
    coder = ResidualCoder()
    for m in ar.MAPS:
        assert DeviceTargetAssigner.supported(ar.head_cfg(m), coder)

    def refused(cfg, word, coder=coder, **kw):
        if not kw:
            assert not DeviceTargetAssigner.supported(cfg, coder)
        with pytest.raises(ValueError, match=word):
            DeviceTargetAssigner(cfg, ar.MAPS["three"]["class_names"], coder, **kw)

    cfg = ar.head_cfg("three")
    cfg.TARGET_ASSIGNER_CONFIG.POS_FRACTION = 0.5
    refused(cfg, "POS_FRACTION")
    cfg = ar.head_cfg("three")
    cfg.TARGET_ASSIGNER_CONFIG.MATCH_HEIGHT = True
    refused(cfg, "MATCH_HEIGHT")
    refused(ar.head_cfg("three"), "MATCH_HEIGHT", match_height=True)
    cfg = ar.head_cfg("three")
    cfg.TARGET_ASSIGNER_CONFIG.NORM_BY_NUM_EXAMPLES = True
    refused(cfg, "NORM_BY_NUM_EXAMPLES")
    refused(ar.head_cfg("three", USE_MULTIHEAD=True), "USE_MULTIHEAD")
    refused(ar.head_cfg("three"), "encode_angle_by_sincos", coder=ResidualCoder(encode_angle_by_sincos=True))
    refused(ar.head_cfg("three"), "code size", coder=ResidualCoder(code_size=9))
    cfg = ar.head_cfg("three")
    cfg.ANCHOR_GENERATOR_CONFIG[1]["anchor_rotations"] = [0]
    refused(cfg, "anchor_rotations")


def test_host_tables_of_three_classes():
    from btcdet_amd.anchor_targets import DeviceTargetAssigner
    from btcdet_amd.dense_head import ResidualCoder
    cfg, names = ar.head_cfg("three"), ar.MAPS["three"]["class_names"]
    a = DeviceTargetAssigner(cfg, names, ResidualCoder())
    assert a.slot_cfg.tolist() == [0, 0, 1, 1, 2, 2] and a.slot_cfg.dtype == np.int32
    assert a.class_cfg.tolist() == [-1, 0, 1, 2, -1], "class 0 wraps to the last name (Van), which has no configuration"
    assert a.matched.tolist() == [np.float32(0.6), 0.5, 0.5] and a.unmatched.tolist() == [np.float32(0.45), np.float32(0.35), np.float32(0.35)]
    for got, want in zip((a.slot_cfg, a.matched, a.unmatched, a.class_cfg), ar.host_tables(cfg, names)):
        assert np.array_equal(got, want) and got.dtype == want.dtype
    one = DeviceTargetAssigner(ar.head_cfg("one"), ["Car"], ResidualCoder())
    assert one.class_cfg.tolist() == [0, 0] and one.slot_cfg.tolist() == [0, 0]
    flat = one.flat_anchors(_anchors("one"))
    assert np.array_equal(flat.numpy(), G["anchors/one"])
    with pytest.raises(ValueError, match="anchor tensors"):
        a.flat_anchors(_anchors("one"))


def test_head_takes_the_device_route_only_when_asked():
    from btcdet_amd.anchor_targets import DeviceTargetAssigner
    from btcdet_amd.dense_head import AnchorHeadSingle, AxisAlignedTargetAssigner
    m = ar.MAPS["one"]

    def head(cfg):
        return AnchorHeadSingle(cfg, input_channels=8, num_class=1, class_names=m["class_names"], grid_size=np.array(m["grid_size"]),
                                point_cloud_range=np.array(m["point_cloud_range"], np.float32))
    assert type(head(ar.head_cfg("one")).target_assigner) is AxisAlignedTargetAssigner
    assert type(head(ar.head_cfg("one", device=False)).target_assigner) is AxisAlignedTargetAssigner
    h = head(ar.head_cfg("one", device=True))
    assert type(h.target_assigner) is DeviceTargetAssigner and h.device_targets
    cfg = ar.head_cfg("one", device=True)
    cfg.TARGET_ASSIGNER_CONFIG.POS_FRACTION = 0.5           # not computed on the device: the torch route, as without the key
    h = head(cfg)
    assert type(h.target_assigner) is AxisAlignedTargetAssigner and not h.device_targets
    for name in ("btcdet_kitti_car.yaml", "btcdet_waymo_synth.yaml"):
        assert "DEVICE" not in open(os.path.join(ROOT, "btcdet_amd", "cfgs", name)).read(), "the shipped configurations stay without the key"


# ------------------------------------------------------------------------------------------------------------------------- C ABI
def test_ctypes_table_matches_the_header():
    from btcdet_amd import _lib
    src = open(os.path.join(ROOT, "include", "btcdet_hip_heads.h")).read()
    for line in ("iou = inter / max((area_a + area_g) - inter, 1e-6)", "q = r * (1/pi) ; lp = r - floor(q + 0.5) * pi ; snapped = |lp| < pi/4",
                 "s_j = (((((x + y) + z) + dx) + dy) + dz) + r", "x = t0 * diag + xa ; y = t1 * diag + ya ; z = t2 * dza + za",
                 "v = rot - dir_offset ; q = v * inv ; lp = v - floor(q + dir_limit_offset) * period"):
        assert line in src, "the header states its formulas: " + line
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.HEADS_EXPORTED_SYMBOLS) == ["btc_anchor_targets", "btc_anchor_targets_ws_bytes", "btc_decode_anchor_boxes"]
    L = _lib.lib()
    kinds = {"int": _lib.ci, "size_t": _lib.sz, "float": _lib.cf}
    for n, count in (("btc_anchor_targets", 18), ("btc_anchor_targets_ws_bytes", 2), ("btc_decode_anchor_boxes", 10)):
        assert hasattr(L, n)
        res, args = _lib._HEADS_SIGS[n]
        m = re.search(r"(size_t|int)\s+%s\s*\(([^)]*)\)" % n, src)
        assert kinds[m.group(1)] is res, n
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args) == count, n
        for p, a in zip(params, args):
            want = _lib.vp if "*" in p else kinds[re.sub(r"\s+\w+$", "", p).replace("const ", "").strip()]
            assert a is want, (n, p)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "btcdet_hip_heads.h":
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
            assert not set(names) & set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", text)), other
    from btcdet_amd import anchor_targets as at
    for k, v in (("BTC_HEADS_MAX_SLOTS", at.MAX_SLOTS), ("BTC_HEADS_MAX_CFGS", at.MAX_CFGS), ("BTC_HEADS_MAX_CLASSES", at.MAX_CLASSES)):
        assert re.search(r"#define %s (\d+)" % k, src).group(1) == str(v)
    assert L.btc_anchor_targets_ws_bytes(0, 4) == 0 and L.btc_anchor_targets_ws_bytes(2, -1) == 0 and L.btc_anchor_targets_ws_bytes(2 ** 20, 2 ** 10) == 0
    assert L.btc_anchor_targets_ws_bytes(2, 0) == 256 and L.btc_anchor_targets_ws_bytes(3, 65) == 256 + 1024


def test_refusals_need_no_device():
    """every refusal happens before any launch, so it can be asked for without a GPU; the device pointers are never read"""
    from btcdet_amd import _lib
    L = _lib.lib()
    slot_cfg, matched, unmatched, class_cfg = ar.host_tables(ar.head_cfg("three"), ar.MAPS["three"]["class_names"])
    fake = 1 << 20
    names = ["anchors", "A", "slots", "slot_cfg", "ncfg", "matched", "unmatched", "class_cfg", "num_class", "gt", "B", "M", "labels", "targets",
             "weights", "ws", "ws_bytes"]
    good = [fake, 12, 6, slot_cfg.ctypes.data, 3, matched.ctypes.data, unmatched.ctypes.data, class_cfg.ctypes.data, 4, fake, 2, 5, fake, fake, fake, fake,
            L.btc_anchor_targets_ws_bytes(2, 5)]
    bad_slot, bad_class = slot_cfg.copy(), class_cfg.copy()
    bad_slot[3], bad_class[2] = 3, -2
    for kw in (dict(B=0), dict(A=-6), dict(M=-1), dict(slots=0), dict(slots=65), dict(A=13), dict(ncfg=0), dict(ncfg=17), dict(num_class=-1),
               dict(num_class=64), dict(slot_cfg=bad_slot.ctypes.data), dict(class_cfg=bad_class.ctypes.data), dict(ncfg=2), dict(slot_cfg=None),
               dict(matched=None), dict(unmatched=None), dict(class_cfg=None), dict(anchors=None), dict(gt=None), dict(labels=None), dict(targets=None),
               dict(weights=None), dict(ws=None), dict(ws_bytes=good[-1] - 1), dict(ws_bytes=0), dict(B=2 ** 20, A=6 * 2 ** 10)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert L.btc_anchor_targets(*a, None) == -1, kw
        assert b"btc_anchor_targets" in L.btc_last_error()
    for args in ((fake, fake, None, 0, 5, 0, 0.0, 0.0, fake), (fake, fake, None, 1, -1, 0, 0.0, 0.0, fake), (None, fake, None, 1, 5, 0, 0.0, 0.0, fake),
                 (fake, None, None, 1, 5, 0, 0.0, 0.0, fake), (fake, fake, None, 1, 5, 0, 0.0, 0.0, None), (fake, fake, fake, 1, 5, 0, 0.0, 0.0, fake),
                 (fake, fake, None, 2 ** 16, 2 ** 13, 0, 0.0, 0.0, fake)):
        assert L.btc_decode_anchor_boxes(*args, None) == -1, args
