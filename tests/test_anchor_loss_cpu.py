"""btcdet_amd/anchor_loss.py without a GPU: the float64 restatement of include/btcdet_hip_anchor_loss.h (anchor_loss_ref.restate) against
the reference's own float64 record (tests/golden/anchor_loss.npz, made by gen_anchor_loss_golden.py) at 1e-12 relative; the reference's
float32 record, the torch route of dense_head.AnchorHeadSingle.get_loss on the CPU and a float32 emulation of the kernels inside the
derived bound; six seeded defects, each caught on a listed case; unsupported_reason, the opt-in key, the ctypes table against the header
and the refusals that need no launch."""
import logging
import os
import re
import types

import numpy as np
import pytest
import torch

import anchor_loss_ref as al
import anchor_targets_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, CASES = al.gold()


def _gold(case):
    return al.gold_case(G, case["name"], case["dir"])


def _record(case, suffix):
    n = case["name"]
    return G[n + "/loss" + suffix], G[n + "/d_cls" + suffix], G[n + "/d_box" + suffix], (G[n + "/d_dir" + suffix] if case["dir"] else None)


def _as_got(d, out, d_cls, d_box, d_dir, g=1.0):
    nb = np.maximum((d["labels"] > 0).sum(1), 1)
    return dict(out=np.asarray(out, np.float32), norms=(1.0 / nb).astype(np.float32), d_cls=d_cls, d_box=d_box, d_dir=d_dir, g=g)


def test_golden_cases_cover_what_they_must():
    names = {c["name"]: c for c in CASES}
    counts = {n: (G[n + "/labels"].astype(np.int32) > 0).sum(1).tolist() for n in names}
    assert {G[n + "/cls"].shape[2] for n in names} == {1, 3} and {c["dir"] for c in CASES} == {True, False}
    assert {G[n + "/cls"].shape[0] for n in names} == {1, 2, 3}
    assert any(0 in v for v in counts.values()) and any(1 in v for v in counts.values())
    assert any(np.all(G[n + "/labels"][b] < 0) for n in names for b in range(G[n + "/labels"].shape[0])), "a scene of ignored anchors only"
    assert any(np.isnan(G[n + "/tgt"][G[n + "/labels"] > 0]).any() for n in names), "a NaN regression target at a positive anchor"
    assert all(G[n + "/anchors"].shape[0] <= 1530 for n in names)
    for c in CASES:                                               # the margins the generator asserted, again on what was recorded
        on = None
        if c["clamp"]:
            on = np.zeros(G[c["name"] + "/labels"].shape, bool)
            on[tuple(c["on_clamp"])] = True
        al.margins_dir(_gold(c), on_clamp=on)
    assert sum(c["clamp"] for c in CASES) == 1


@pytest.mark.parametrize("case", [c for c in CASES if c["f64"]], ids=lambda c: c["name"])
def test_restatement_equals_the_float64_record(case):
    R = al.restate(_gold(case), own=True)
    for got, ref in zip((R["out"], R["d_cls"], R["d_box"], R["d_dir"]), _record(case, "64")):
        if ref is None:
            assert got is None
            continue
        assert ref.dtype == np.float64 and np.isfinite(ref).all()
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_float32_record_lies_inside_the_bound(case):
    d = _gold(case)
    W = al.Worst()
    al.check_anchor(W, d, _as_got(d, *_record(case, "32")), case["name"])
    print(case["name"], W.report())


def _torch_route(d, dtype=torch.float32):
    """dense_head.AnchorHeadSingle.get_loss, torch formulation, on the recorded (B, A, *) tensors"""
    from btcdet_amd.dense_head import AnchorHeadSingle
    B, A, C = d["cls"].shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    f = dict(cls_preds=t(d["cls"]).requires_grad_(True), box_preds=t(d["box"]).requires_grad_(True), box_cls_labels=torch.from_numpy(d["labels"].copy()),
             box_reg_targets=t(d["tgt"]))
    cfg = ar.ED(LOSS_CONFIG=dict(LOSS_WEIGHTS=dict(d["w"])), NUM_DIR_BINS=2, DIR_OFFSET=d["dir_offset"])
    if d["dir"] is not None:
        f["dir_cls_preds"] = t(d["dir"]).requires_grad_(True)
    anchors = torch.from_numpy(d["anchors"])
    me = types.SimpleNamespace(forward_ret_dict=f, model_cfg=cfg, num_class=C, num_anchors_per_location=1, device_loss=False,
                               _flat_anchors=lambda dev, bs: anchors.view(1, A, 7).repeat(bs, 1, 1))
    loss, tb = AnchorHeadSingle.get_loss(me)
    loss.backward()
    out = [float(tb["rpn_loss_cls"]), float(tb["rpn_loss_loc"]), float(tb.get("rpn_loss_dir", 0.0)), float(tb["rpn_loss"])]
    g = lambda k: f[k].grad.numpy() if k in f else None
    return out, g("cls_preds"), g("box_preds"), g("dir_cls_preds"), list(tb)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_torch_route_on_cpu_lies_inside_the_bound(case):
    d = _gold(case)
    out, d_cls, d_box, d_dir, keys = _torch_route(d)
    assert keys == ["rpn_loss_cls", "rpn_loss_loc"] + (["rpn_loss_dir"] if case["dir"] else []) + ["rpn_loss"]
    W = al.Worst()
    al.check_anchor(W, d, _as_got(d, out, d_cls, d_box, d_dir), case["name"])
    print(case["name"], W.report())


EMULATED = al.shape_cases() + al.value_cases() + al.cap_cases()[:1]


def test_emulation_lies_inside_the_bound():
    """the float32 emulation of both launches over the case lists the GPU tests run (poisoned: NaN wherever the labels exclude)"""
    W = al.Worst()
    for c in EMULATED:
        d = al.make_case(c)
        al.check_anchor(W, d, al.emulate(d), al.case_name(c))
    for c in CASES:
        d = _gold(c)
        al.check_anchor(W, d, al.emulate(d), c["name"])
    print(W.report())


@pytest.mark.parametrize("defect", al.DEFECTS)
def test_the_checks_can_fail(defect):
    """every seeded defect exceeds a bound (or breaks an exact property) on at least one listed case.  beta_ulp is caught by the exact
    seam property on the beta_seam cases: a one-ulp change of beta moves every value by about u, below any derived bound"""
    caught = []
    cases = [(al.case_name(c), al.make_case(c)) for c in al.value_cases() + [dict(B=3, A=257, C=3, bins=2, kind="random")]] + \
            [(c["name"], _gold(c)) for c in CASES]
    for name, d in cases:
        W = al.Worst(strict=False)
        al.check_anchor(W, d, al.emulate(d, defect=defect), name)
        if max(W.worst.values()) > 1.0:
            caught.append((name, {k: v for k, v in W.worst.items() if v > 1.0}))
    print(defect, "caught on %d of %d cases, e.g." % (len(caught), len(cases)), caught[:2])
    assert caught, defect


def test_poison_changes_nothing_in_the_restatement():
    for c in al.value_cases()[:4]:
        a, b = al.restate(al.make_case(c, poison=True)), al.restate(al.make_case(c, poison=False))
        for k in ("out", "d_cls", "d_box"):
            assert np.array_equal(a[k], b[k]), (c, k)


# ------------------------------------------------------------------------------------------------------------------------- the module
def test_unsupported_reason_names_the_bar():
    from btcdet_amd import anchor_loss
    from btcdet_amd.dense_head import ResidualCoder
    cfg = al.gold_cfg("car")
    assert anchor_loss.unsupported_reason(cfg, ResidualCoder(), 1) is None
    assert anchor_loss.unsupported_reason(al.gold_cfg("car", with_dir=False), ResidualCoder(), 3) is None
    assert "USE_MULTIHEAD" in anchor_loss.unsupported_reason(ar.ED(dict(cfg, USE_MULTIHEAD=True)), ResidualCoder(), 1)
    assert "encode_angle_by_sincos" in anchor_loss.unsupported_reason(cfg, ResidualCoder(encode_angle_by_sincos=True), 1)
    assert "code size of 9" in anchor_loss.unsupported_reason(cfg, ResidualCoder(code_size=9), 1)
    assert "classes" in anchor_loss.unsupported_reason(cfg, ResidualCoder(), anchor_loss.MAX_CLASSES)
    assert "NUM_DIR_BINS" in anchor_loss.unsupported_reason(ar.ED(dict(cfg, NUM_DIR_BINS=anchor_loss.MAX_BINS + 1)), ResidualCoder(), 1)
    assert anchor_loss.unsupported_reason(ar.ED(dict(cfg, NUM_DIR_BINS=anchor_loss.MAX_BINS)), ResidualCoder(), anchor_loss.MAX_CLASSES - 1) is None
    with pytest.raises(ValueError, match="no CPU fallback"):
        anchor_loss.anchor_loss(torch.zeros(1, 2, 1), torch.zeros(1, 2, 7), None, torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, 7), torch.zeros(2, 7),
                                al.W_DEFAULT)


def _head(cfg, map_name="car"):
    from btcdet_amd.dense_head import AnchorHeadSingle
    m = al.GOLD_MAPS[map_name]
    torch.manual_seed(3)
    return AnchorHeadSingle(cfg, input_channels=8, num_class=len(m["class_names"]), class_names=m["class_names"], grid_size=np.array(m["grid_size"]),
                            point_cloud_range=np.array(m["point_cloud_range"], np.float32))


def _fill(head, case):
    d = _gold(case)
    B, A, _ = d["cls"].shape
    per = head.num_anchors_per_location
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).view(B, 8, 8, -1).requires_grad_(True)
    head.forward_ret_dict = dict(cls_preds=t(d["cls"]), box_preds=t(d["box"]), dir_cls_preds=t(d["dir"]), box_cls_labels=torch.from_numpy(d["labels"].copy()),
                                 box_reg_targets=torch.from_numpy(d["tgt"]))
    assert per * 64 == A
    return head.forward_ret_dict


def test_cpu_tensors_keep_the_torch_route_and_the_key_is_opt_in(caplog):
    case = [c for c in CASES if c["name"] == "car_dir_b3_mixed"][0]
    plain, keyed = _head(al.gold_cfg("car")), _head(al.gold_cfg("car", DEVICE=True))
    assert not plain.device_loss and keyed.device_loss
    assert not _head(al.gold_cfg("car", DEVICE=False)).device_loss
    res = []
    for h in (plain, keyed):
        f = _fill(h, case)
        loss, tb = h.get_loss()
        loss.backward()
        res.append((loss.detach().numpy(), {k: float(v) for k, v in tb.items()}, [f[k].grad.numpy() for k in ("cls_preds", "box_preds", "dir_cls_preds")]))
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1], "CPU tensors: the keyed head gives the bits of the torch route"
    assert all(np.array_equal(a, b) for a, b in zip(res[0][2], res[1][2]))
    assert list(res[0][1]) == ["rpn_loss_cls", "rpn_loss_loc", "rpn_loss_dir", "rpn_loss"]
    # an unsupported configuration keeps the torch route and says why, once, at construction
    cfg = al.gold_cfg("car", DEVICE=True)
    cfg.NUM_DIR_BINS = 17
    with caplog.at_level(logging.WARNING, logger="btcdet_amd.dense_head"):
        h = _head(cfg)
    assert not h.device_loss
    said = [r.getMessage() for r in caplog.records if "LOSS_CONFIG.DEVICE" in r.getMessage()]
    assert len(said) == 1 and "NUM_DIR_BINS" in said[0] and "torch route" in said[0]
    for name in ("btcdet_kitti_car.yaml", "btcdet_waymo_synth.yaml"):
        text = open(os.path.join(ROOT, "btcdet_amd", "cfgs", name)).read()
        assert "DEVICE" not in text, "the shipped configurations stay without the key"


# ------------------------------------------------------------------------------------------------------------------------- C ABI
def test_ctypes_table_matches_the_header():
    from btcdet_amd import _lib, anchor_loss
    src = open(os.path.join(ROOT, "include", "btcdet_hip_anchor_loss.h")).read()
    for line in ("e = expf(-|x|) ; r = 1 / (1 + e) ; p = x >= 0 ? r : e * r ; om = 1 - p", "term = (alpha_t * (pt * pt)) * bce",
                 "d = u - v ; n = |d| ; term = n < beta ? 0.5 * (n * n) / beta : n - 0.5 * beta",
                 "rot = t_6 + anchor_6 ; v = rot - dir_offset ; q = v * (1 / two_pi) ; lp = v - floor(q) * two_pi",
                 "out[3]      = out[0] + (out[1] + out[2]) in float32", "norms[b]    = float32(1 / n_b)"):
        assert line in src, "the header states its formulas: " + line
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.ANCHOR_LOSS_EXPORTED_SYMBOLS) == ["btc_anchor_loss_bwd", "btc_anchor_loss_fwd", "btc_anchor_loss_ws_bytes"]
    L = _lib.lib()
    kinds = {"int": _lib.ci, "size_t": _lib.sz, "float": _lib.cf}
    for n, count in (("btc_anchor_loss_fwd", 19), ("btc_anchor_loss_bwd", 20), ("btc_anchor_loss_ws_bytes", 2)):
        assert hasattr(L, n)
        res, args = _lib._ANCHOR_LOSS_SIGS[n]
        m = re.search(r"(size_t|int)\s+%s\s*\(([^)]*)\)" % n, src)
        assert kinds[m.group(1)] is res, n
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args) == count, n
        for p, a in zip(params, args):
            want = _lib.vp if "*" in p else kinds[re.sub(r"\s+\w+$", "", p).replace("const ", "").strip()]
            assert a is want, (n, p)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "btcdet_hip_anchor_loss.h":
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
            assert not set(names) & set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", text)), other
    for k, v in (("BTC_ANCHOR_LOSS_THREADS", al.THREADS), ("BTC_ANCHOR_LOSS_MAX_TILES", al.MAX_TILES), ("BTC_ANCHOR_LOSS_MAX_BINS", al.MAX_BINS)):
        assert re.search(r"#define %s (\d+)" % k, src).group(1) == str(v)
    assert (anchor_loss.THREADS, anchor_loss.MAX_TILES, anchor_loss.MAX_BINS, anchor_loss.MAX_CLASSES) == (al.THREADS, al.MAX_TILES, al.MAX_BINS, al.MAX_CLASSES)
    ws = L.btc_anchor_loss_ws_bytes
    assert ws(0, 4) == 0 and ws(2, -1) == 0 and ws(2 ** 16, 2 ** 13) == 0
    assert ws(1, 0) == 256 + 32 and ws(3, 257) == 256 + 3 * 2 * 32 and ws(2, 70400) == 256 + 2 * 275 * 32
    assert ws(1, al.CAP) == ws(1, al.CAP + 1) == ws(1, 10 ** 7) == 256 + al.MAX_TILES * 32


def test_refusals_need_no_device():
    """every refusal happens before any launch, so it can be asked for without a GPU; the device pointers are never read"""
    from btcdet_amd import _lib
    L = _lib.lib()
    fake = 1 << 20
    B, A, C, bins = 2, 300, 3, 2
    ws_bytes = L.btc_anchor_loss_ws_bytes(B, A)
    fwd = dict(cls=fake, box=fake, dir=fake, labels=fake, tgt=fake, anchors=fake, B=B, A=A, C=C, bins=bins, cw=1.0, lw=2.0, dw=0.2, off=0.78539, out=fake,
               norms=fake, ws=fake, ws_bytes=ws_bytes)
    bwd = dict(list(fwd.items())[:14], norms=fake, grad=fake, d_cls=fake, d_box=fake, d_dir=fake)
    common = [dict(B=0), dict(B=-1), dict(A=-1), dict(C=0), dict(C=64), dict(bins=-1), dict(bins=17), dict(cls=None), dict(box=None), dict(dir=None),
              dict(labels=None), dict(tgt=None), dict(anchors=None), dict(B=2 ** 12, A=2 ** 17)]
    for fn, good, extra in ((L.btc_anchor_loss_fwd, fwd, [dict(out=None), dict(norms=None), dict(ws=None), dict(ws_bytes=ws_bytes - 1), dict(ws_bytes=0)]),
                            (L.btc_anchor_loss_bwd, bwd, [dict(norms=None), dict(grad=None), dict(d_cls=None), dict(d_box=None), dict(d_dir=None)])):
        for kw in common + extra:
            a = dict(good, **kw)
            assert fn(*a.values(), None) == -1, kw
            assert L.btc_last_error().decode().startswith("btc_anchor_loss_"), kw
    # legal and launching nothing: the backward over no anchors; a NULL dir with bins = 0 is no refusal either (checked on the GPU)
    assert L.btc_anchor_loss_bwd(*dict(bwd, A=0, cls=None, box=None, dir=None, labels=None, tgt=None, anchors=None, d_cls=None, d_box=None, d_dir=None).values(), None) == 0
