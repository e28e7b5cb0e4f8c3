"""btcdet_amd/roi_targets_device.py without a GPU: the numpy restatement of include/btcdet_hip_roi_targets.h (roi_targets_ref) against
roi_targets.sample_rois on CPU tensors with the same uniforms, against the reference's own record of the labels and the canonical
transform (tests/golden/roi_targets.npz), its case lists (margins clear, foreground keys distinct, every kind of scene present), the
seeded defects, the ctypes table against the header, and the refusals -- which happen before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import roi_targets_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 128


def _gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "roi_targets.npz"))


# ------------------------------------------------------------------------------------------------------------------- the sampler
def _sampler_vectors():
    for seed in range(12):
        yield "seed%d" % seed, rr.sampler_overlaps(seed)
    for n in (1, R - 1, R, R + 1):
        for seed in (0, 1, 2, 3, 5):
            yield "n%d_kind%d" % (n, seed % 6), rr.sampler_overlaps(seed, n)


@pytest.mark.parametrize("name,ov", list(_sampler_vectors()), ids=[n for n, _ in _sampler_vectors()])
def test_restated_sampling_equals_sample_rois(name, ov):
    from btcdet_amd.roi_targets import sample_rois
    import common
    M = max(R, ov.shape[0])
    u = common._hash01(4 * M, 900 + ov.shape[0]).reshape(4, M)
    fg_keys = u[0, :ov.shape[0]][ov >= np.float32(0.55)]
    assert np.unique(fg_keys).size == fg_keys.size
    want = sample_rois(torch.from_numpy(ov), rr.SAMPLER_CFG, uniforms=torch.from_numpy(u)).numpy()
    got = rr.sample(ov, u, rr.SAMPLER_CFG)
    assert got.dtype == np.int64 and np.array_equal(got, want)


def test_sample_rois_without_uniforms_draws_as_before():
    """the optional argument changes nothing when absent: the generator's stream is consumed exactly as it was"""
    from btcdet_amd.roi_targets import sample_rois
    ov = torch.from_numpy(rr.sampler_overlaps(0))
    a = sample_rois(ov, rr.SAMPLER_CFG, torch.Generator().manual_seed(4))
    u = torch.rand((4, max(R, ov.shape[0])), generator=torch.Generator().manual_seed(4))
    assert torch.equal(a, sample_rois(ov, rr.SAMPLER_CFG, uniforms=u))


# ------------------------------------------------------------------------------------------------- the reference's record (golden)
def test_restated_labels_and_transform_vs_reference_record():
    """the conditions of tests/test_hip_roi_targets.py: atol 2e-5, rows within 1e-4 of a threshold left out, at most 1 % of them"""
    g = _gold()
    cfg = rr.make_cfg()
    iou = g["t_gt_iou_of_rois"]
    clear = np.ones_like(iou, bool)
    for th in (cfg.REG_FG_THRESH, cfg.CLS_FG_THRESH, cfg.CLS_BG_THRESH):
        clear &= np.abs(iou - th) > 1e-4
    assert clear.mean() > 0.99
    for dt in (np.float32, np.float64):
        reg, cls = rr.labels_of(iou, cfg, dt)
        assert np.array_equal(reg[clear], g["t_reg_valid_mask"][clear])
        np.testing.assert_allclose(cls[clear], g["t_rcnn_cls_labels"][clear], rtol=0, atol=1e-4)
        np.testing.assert_allclose(rr.canonical(g["t_rois"], g["t_gt_of_rois_src"], dt), g["t_gt_of_rois"], rtol=0, atol=2e-5)
    # the emulation against the float64 values, inside the derived bound; everything but the rotated columns: the same bits
    emu, ref = rr.canonical(g["t_rois"], g["t_gt_of_rois_src"], np.float32), rr.canonical(g["t_rois"], g["t_gt_of_rois_src"], np.float64)
    assert (np.abs(emu[..., :2].astype(np.float64) - ref[..., :2]) <= rr.rotated_bound(g["t_rois"], g["t_gt_of_rois_src"])).all()
    assert np.array_equal(emu[..., 2], g["t_gt_of_rois"][..., 2]) and np.array_equal(emu[..., 7], g["t_gt_of_rois"][..., 7])


# ----------------------------------------------------------------------------------------------------------------- the case lists
@pytest.fixture(scope="module")
def runs():
    out = {}
    for spec in rr.CASES:
        case = rr.make_case(spec)
        out[spec["name"]] = (case, rr.analytic_bev(case))
    return out


def test_case_lists_cover_what_they_claim(runs):
    seen = dict(fg_only=False, easy_only=False, hard_only=False, no_fg=False, zero=False, alien=False, at_integer=False)
    n_fgs, Ns, Gs, Bs = set(), set(), set(), set()
    for name, (case, bev) in runs.items():
        cfg = case["cfg"]
        emu = rr.restate(case, bev, np.float32)
        m = rr.margins(emu["max_overlaps"], emu["gt_iou_of_rois"], case["uniforms"], cfg)
        assert rr.clear(m), (name, m)
        assert rr.foreground_keys_distinct(emu["max_overlaps"], case["uniforms"], cfg), name
        assert (m["hard_num"] == 0.0) == (name in rr.HARD_NUM_AT_INTEGER), (name, m)
        seen["at_integer"] |= m["hard_num"] == 0.0
        B, N = case["rois"].shape[:2]
        Ns.add(N), Gs.add(case["gt_boxes"].shape[1]), Bs.add(B)
        c = rr.consts(cfg)
        for b in range(B):
            ov = emu["max_overlaps"][b]
            # the closed-form kinds are what the restated IoU says they are
            assert np.array_equal(ov >= c.fg_thresh, case["kinds"][b] == 2) or case["spec"]["alien_scene"] == b and cfg.SAMPLE_ROI_BY_EACH_CLASS, name
            n_fg, n_easy = int((ov >= c.fg_thresh).sum()), int((ov < c.cls_bg_lo).sum())
            n_hard = N - n_fg - n_easy
            if cfg.ROI_PER_IMAGE == R:
                n_fgs.add(n_fg)
            seen["fg_only"] |= n_fg == N
            seen["easy_only"] |= n_easy == N
            seen["hard_only"] |= n_hard == N
            seen["no_fg"] |= n_fg == 0 and n_hard > 0 and n_easy > 0
            seen["zero"] |= not case["gt_boxes"][b].any()
            seen["alien"] |= bool(cfg.SAMPLE_ROI_BY_EACH_CLASS) and not (case["roi_labels"][b][:, None] == case["gt_boxes"][b][None, :, 7]).any()
            sel = emu["sampled_inds"][b]
            assert sel.min() >= 0 and sel.max() < N
    assert all(seen.values()), seen
    assert {63, 64, 65} <= n_fgs and {1, 63, 64, 65, R - 1, R, 257, 512, 1024} <= Ns and Gs == {1, 2, 37} and Bs >= {1, 3}
    assert {c["by_class"] for c in rr.CASES} == {True, False} and {c["score"] for c in rr.CASES} == {"roi_iou", "cls"}


def test_tie_break_takes_the_lowest_box(runs):
    for name in ("tie", "tie_any_class"):
        case, bev = runs[name]
        assert np.array_equal(case["gt_boxes"][0, 0], case["gt_boxes"][0, 1]) and np.array_equal(bev[0, :, 0], bev[0, :, 1])
        emu = rr.restate(case, bev, np.float32)
        assert (emu["gt_assignment"] == 0).all() and (emu["max_overlaps"] > 0).any()


def test_float32_emulation_inside_the_bound_of_the_float64_values(runs):
    for name, (case, bev) in runs.items():
        emu, ref = rr.restate(case, bev, np.float32), rr.restate(case, bev, np.float64)
        for k in ("gt_assignment", "sampled_inds", "rois", "gt_of_rois_src", "roi_scores", "roi_labels", "reg_valid_mask"):
            assert rr.same_bits(emu[k], ref[k]), (name, k)
        rr.check_outputs(emu, emu, ref, name)
        np.testing.assert_allclose(emu["gt_of_rois"][..., 6], ref["gt_of_rois"][..., 6], rtol=0, atol=1e-5)


@pytest.mark.parametrize("defect", rr.DEFECTS)
def test_each_seeded_defect_fails_on_a_listed_case(runs, defect):
    caught = []
    for name, (case, bev) in runs.items():
        emu, ref = rr.restate(case, bev, np.float32), rr.restate(case, bev, np.float64)
        bad = rr.restate(case, bev, np.float32, defect=defect)
        try:
            rr.check_outputs(bad, emu, ref, name)
        except AssertionError:
            caught.append(name)
    if defect == "reg_valid_ge":
        # `>=` for `>` shows only AT the threshold: the listed label values sit on it
        cfg = rr.make_cfg()
        iou = np.array([np.float32(cfg.REG_FG_THRESH), np.nextafter(np.float32(cfg.REG_FG_THRESH), np.float32(1)), np.float32(0.3)], np.float32)
        good, bad = rr.labels_of(iou, cfg)[0], rr.labels_of(iou, cfg, defect=defect)[0]
        assert good.tolist() == [0, 1, 0] and bad.tolist() == [1, 1, 0]
        assert np.array_equal(good, (torch.from_numpy(iou) > cfg.REG_FG_THRESH).long().numpy())
        return
    assert caught, "no listed case sees the defect %s" % defect


# ------------------------------------------------------------------------------------------------------------------------- C ABI
def test_ctypes_table_matches_the_header():
    from btcdet_amd import _lib, roi_targets_device as rtd
    src = open(os.path.join(ROOT, "include", "btcdet_hip_roi_targets.h")).read()
    for line in ("o3 = o * h ; vol = (dx * dy) * dz ; iou = o3 / max((vol_a + vol_b) - o3, 1e-6f)",
                 "fg_this  = n_bg > 0 ? min(n_fg, fg_quota) : (n_fg > 0 ? R : 0) ; m = R - fg_this",
                 "draw(row, n)[j] = min((long) floor((double) uniforms[b, row, j] * (double) n), max(n, 1) - 1)",
                 "c = cosf(-ry), s = sinf(-ry) ; x' = lx * c - ly * s ; y' = lx * s + ly * c", "among equal values the LOWEST box index wins"):
        assert line in src, "the header states its formulas: " + line
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", code)))
    assert names == sorted(_lib.ROI_TARGETS_EXPORTED_SYMBOLS) == ["btc_roi_targets", "btc_roi_targets_ws_bytes"]
    L = _lib.lib()
    kinds = {"int": _lib.ci, "size_t": _lib.sz}
    for n, count in (("btc_roi_targets", 24), ("btc_roi_targets_ws_bytes", 2)):
        assert hasattr(L, n)
        res, args = _lib._ROI_TARGETS_SIGS[n]
        m = re.search(r"(size_t|int)\s+%s\s*\(([^)]*)\)" % n, code)
        assert kinds[m.group(1)] is res, n
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args) == count, n
        for p, a in zip(params, args):
            if "BtcRoiTargetsConfig" in p:
                assert a is ctypes.POINTER(_lib.BtcRoiTargetsConfig)
            else:
                assert a is (_lib.vp if "*" in p else kinds[re.sub(r"\s+\w+$", "", p).strip()]), (n, p)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "btcdet_hip_roi_targets.h":
            text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
            assert not set(names) & set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", text)), other
    # the struct: the header's fields in the header's order, C layout
    body = re.search(r"typedef struct BtcRoiTargetsConfig \{(.*?)\}", code, flags=re.S).group(1)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in re.sub(r"^\s*(int32_t|float|double)\s+", "", decl.strip()).split(",")]
    assert fields == [f[0] for f in _lib.BtcRoiTargetsConfig._fields_] and ctypes.sizeof(_lib.BtcRoiTargetsConfig) == 48
    for k, v in (("BTC_ROI_TARGETS_MAX_N", rtd.MAX_N), ("BTC_ROI_TARGETS_MAX_R", rtd.MAX_R), ("BTC_ROI_SCORE_ROI_IOU", rtd.SCORE_TYPES["roi_iou"]),
                 ("BTC_ROI_SCORE_CLS", rtd.SCORE_TYPES["cls"])):
        assert re.search(r"#define %s (\d+)" % k, code).group(1) == str(v)
    assert (rr.MAX_N, rr.MAX_R) == (rtd.MAX_N, rtd.MAX_R)
    ws = L.btc_roi_targets_ws_bytes
    assert ws(0, 4) == 0 and ws(2, 0) == 0 and ws(2, 1025) == 0 and ws(2 ** 20, 1024) == 0
    assert ws(1, 1) == 256 and ws(64, 1024) == 256 and ws(65, 512) == 512


def test_config_block_rounds_on_the_host():
    from btcdet_amd.roi_targets_device import config_block
    blk, c = config_block(rr.make_cfg(FG_RATIO=0.3, ROI_PER_IMAGE=100)), rr.consts(rr.make_cfg(FG_RATIO=0.3, ROI_PER_IMAGE=100))
    assert (blk.R, blk.fg_quota, blk.by_class, blk.score_type) == (100, 30, 1, 0)
    for k in ("reg_fg", "cls_fg", "cls_bg", "cls_bg_lo", "fg_thresh", "cls_span"):
        assert np.float32(getattr(blk, k)) == c[k], k
    assert blk.fg_thresh == blk.reg_fg and blk.hard_bg_ratio == 0.8


def _good_args(**kw):
    from btcdet_amd import _lib
    from btcdet_amd.roi_targets_device import config_block
    fake = 1 << 20
    B, N, G = 2, 300, 5
    blk = config_block(rr.make_cfg())
    for k in ("R", "fg_quota", "score_type"):
        if k in kw:
            setattr(blk, k, kw.pop(k))
    a = dict(rois=fake, scores=fake, labels=fake, gts=fake, uniforms=fake, sampled_in=None, B=B, N=N, G=G, cfg=ctypes.byref(blk), rois_out=fake, gt=fake,
             gt_src=fake, iou=fake, scores_out=fake, labels_out=fake, reg_valid=fake, cls=fake, max_overlaps=fake, gt_assignment=fake, sampled=fake, ws=fake,
             ws_bytes=_lib.lib().btc_roi_targets_ws_bytes(B, N))
    a.update(kw)
    return a, blk


REFUSALS = [dict(B=0), dict(N=0), dict(N=1025), dict(G=0), dict(R=0), dict(R=1025), dict(fg_quota=-1), dict(fg_quota=129), dict(score_type=2), dict(cfg=None),
            dict(rois=None), dict(scores=None), dict(labels=None), dict(gts=None), dict(uniforms=None), dict(sampled_in=1 << 20), dict(rois_out=None), dict(gt=None),
            dict(gt_src=None), dict(iou=None), dict(scores_out=None), dict(labels_out=None), dict(reg_valid=None), dict(cls=None), dict(max_overlaps=None),
            dict(gt_assignment=None), dict(sampled=None), dict(ws=None), dict(ws_bytes=255), dict(ws_bytes=0), dict(B=2 ** 19, N=1024), dict(G=2 ** 28)]


def test_refusals_need_no_device():
    """every refusal happens before any launch, so it can be asked for without a GPU; the device pointers are never read"""
    from btcdet_amd import _lib
    L = _lib.lib()
    for kw in REFUSALS:
        a, blk = _good_args(**dict(kw))
        assert L.btc_roi_targets(*a.values(), None) == -1, kw
        assert L.btc_last_error().decode().startswith("btc_roi_targets"), kw


# --------------------------------------------------------------------------------------------------------------- the Python layer
def test_switch_and_refusal_of_cpu_tensors(caplog):
    import logging
    from btcdet_amd import roi_targets_device as rtd
    assert rtd.unsupported_reason(rr.make_cfg()) is None
    assert "ROI_PER_IMAGE" in rtd.unsupported_reason(rr.make_cfg(ROI_PER_IMAGE=2000))
    assert "CLS_SCORE_TYPE" in rtd.unsupported_reason(rr.make_cfg(CLS_SCORE_TYPE="raw_roi_iou"))
    case = rr.make_case(rr.CASES[1])
    bd = {k: torch.from_numpy(case[k]) for k in ("rois", "roi_scores", "roi_labels", "gt_boxes")}
    bd["batch_size"] = case["batch_size"]
    assert not rtd.usable(bd)
    with pytest.raises(ValueError, match="no CPU fallback"):
        rtd.DeviceProposalTargets(case["cfg"])(bd)
    with pytest.raises(ValueError, match="ROI_PER_IMAGE"):
        rtd.DeviceProposalTargets(rr.make_cfg(ROI_PER_IMAGE=2000))
    for name in ("btcdet_kitti_car.yaml", "btcdet_waymo_synth.yaml"):
        assert "DEVICE" not in open(os.path.join(ROOT, "btcdet_amd", "cfgs", name)).read(), "the shipped configurations stay without the key"
