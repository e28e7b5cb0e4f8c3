"""`bm_points` formed on the GPU from a resident TemplateBank (DeviceAugmentor with `templates`, csrc/best_match.hip) against the
reference's own bytes (tests/golden/best_match.npz: its DataAugmentor.forward with its MltBestMatchQuerier) and, for hand-made
placements through the C ABI, against the numpy restatement of include/btcdet_hip_bestmatch.h (best_match_cases, itself held to
np.einsum and to the golden bytes by tests/test_best_match_cpu.py).  The expectation is never the device code, and everything is
compared EXACTLY (bytes).

  whole path   the three scenes as one batch and as three batches of one, both queue orders: special["bm_points"] per scene, the
               indexed (n, 4) form against collate_batch's, the scan against the recorded digest
  placements   templates of 0 / 1 / 255 / 256 / 257 rows; 44 against 45 rows a scene; an empty scene between two others; scene and
               placement boundaries inside a workgroup; more placements in a workgroup than it stages; one template twice; -0.0;
               out_ld 3 and 4 (aligned or not); no op; rows outside the bank
  fallback     a float64-box scene inside a batch: per scene, in scene order
  sync=False   under torch.cuda.set_sync_debug_mode("error")"""
import os

import numpy as np
import pytest
import torch

import augment_cases as ac
import best_match_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(got.shape[0], -1).any(axis=1))[0]
        raise AssertionError("%s: %d of %d rows differ, first %d: got %s want %s" % (what, bad.size, got.shape[0], bad[0], got[bad[0]], want[bad[0]]))


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "best_match.npz"))


def _resident(scenes):
    pts = torch.from_numpy(np.concatenate([s["points"] for s in scenes])).to(DEV)
    offs = torch.from_numpy(np.cumsum([0] + [s["points"].shape[0] for s in scenes]).astype(np.int32)).to(DEV)
    return pts, offs


@pytest.mark.parametrize("grouping", ["one_batch", "three_batches"])
@pytest.mark.parametrize("order", list(bc.ORDERS))
def test_whole_path_equals_the_reference(tmp_path, order, grouping):
    from btcdet_amd import collate
    from btcdet_amd.device_augmentor import DeviceAugmentor, TemplateBank
    g = golden()
    aug, bank, arrays, roots = bc.build(tmp_path, order)
    dev_aug = DeviceAugmentor(aug, bank, TemplateBank(roots))
    scenes = bc.scenes()
    groups = [scenes] if grouping == "one_batch" else [[s] for s in scenes]
    np.random.seed(ac.SEED)
    i = 0
    for grp in groups:
        pts, offs = _resident(grp)
        plan = dev_aug.plan(grp)
        assert plan.bm_device == [True] * len(grp) and not any("bm_points" in s for s in plan.special)
        res = dev_aug.apply(pts, offs, plan, indexed_bm=True)
        t, so = res["special"]["bm_points"]
        assert t.shape == (plan.bm_rows_total, 3) and so.dtype == np.int32 and so[-1] == t.shape[0]
        bounds = res["scene_offsets"].cpu().numpy()
        want = []
        for b in range(len(grp)):
            p = "%s%d_" % (order, i + b)
            want.append(g[p + "bm_points"])
            _same(t[so[b]:so[b + 1]].cpu().numpy(), want[b], (order, grouping, i + b, "bm_points"))
            scan = res["points"][bounds[b]:bounds[b + 1]].cpu().numpy()
            assert np.array_equal(ac.common.sha1(scan), g[p + "points__sha1"]), (order, grouping, i + b, "points")
        _same(res["bm_points"].cpu().numpy(), collate.collate_batch([{"bm_points": w, "is_train": True} for w in want])["bm_points"],
              (order, grouping, i, "indexed"))
        plain = dev_aug.apply(pts, offs, plan)                      # the (n, 3) launch gives the same rows, and no indexed key
        assert "bm_points" not in plain and plain["special"]["bm_points"][0].is_contiguous()
        _same(plain["special"]["bm_points"][0].cpu().numpy(), np.concatenate(want), (order, grouping, i, "out_ld 3"))
        i += len(grp)
    assert np.random.random() == float(g[order + "_rng_next"])


# ------------------------------------------------------------------------------------------------- placements through the C ABI
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cos_sin(angle):
    a = torch.from_numpy(np.array([angle])).float()
    return float(torch.cos(a)[0]), float(torch.sin(a)[0])


def _place(rng, yaw=None):
    from btcdet_amd import data_side
    yaw = np.float32(rng.uniform(-3.1, 3.1) if yaw is None else yaw)
    R = data_side.get_yaw_rotation(yaw)
    c = rng.uniform((0, -30, -2), (60, 30, 0)).astype(np.float32)
    return [R[0, 0], R[0, 1], R[1, 0], c[0], c[1], c[2], 0.0, 0.0]


def _ops(rows, flip=True, scale=1.03125, angle=0.3, order="fsr"):
    """a scene's op program with the flag its bm_points row count asks for"""
    flag = 1.0 if rows < 45 else 0.0
    out = []
    for ch in order:
        if ch == "f" and flip:
            out.append((1, 0, 0, flag))
        elif ch == "s" and scale is not None:
            out.append((2, np.float32(scale), 0, flag))
        elif ch == "r" and angle is not None:
            out.append((3,) + _cos_sin(angle) + (flag,))
    return out


def run_placements(bank, per_scene, ops, out_ld, misalign=False):
    """btc_place_templates with hand-made placements.  per_scene: list (scenes) of lists of (first, rows, place[8]); ops: list of lists of
    (kind, a, b, flag) -> ((n_out + 3, out_ld) array whose last three rows must still be NaN, the restatement (n_out, out_ld))"""
    from btcdet_amd._lib import check, lib, ptr, stream_ptr
    flat = [p for per in per_scene for p in per]
    first, rows = np.array([p[0] for p in flat], np.int32), np.array([p[1] for p in flat], np.int32)
    place = np.array([p[2] for p in flat], np.float32).reshape(-1, 8)
    bm_offs = np.cumsum([0] + [len(per) for per in per_scene]).astype(np.int32)
    row_offs = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    op_rows = np.array([o for per in ops for o in per], np.float32).reshape(-1, 4)
    op_offs = np.cumsum([0] + [len(per) for per in ops]).astype(np.int32)
    n_out = int(row_offs[-1])
    d = dict(bank=_t(bank), first=_t(first) if flat else None, rows=_t(rows) if flat else None, place=_t(place) if flat else None, bm_offs=_t(bm_offs),
             row_offs=_t(row_offs), ops=_t(op_rows) if op_rows.size else None, op_offs=_t(op_offs))
    raw = torch.full(((n_out + 3) * out_ld + 1,), float("nan"), device=DEV)
    out = raw[1:] if misalign else raw[:-1]                    # (one float off a 16-byte boundary: the scalar store path of out_ld 4)
    check(lib().btc_place_templates(ptr(d["bank"]), bank.shape[0], ptr(d["first"]), ptr(d["rows"]), ptr(d["place"]), ptr(d["bm_offs"]), ptr(d["row_offs"]),
                                    len(flat), len(per_scene), ptr(d["ops"]), ptr(d["op_offs"]), n_out, out_ld, out.data_ptr() if n_out else None,
                                    stream_ptr()), "btc_place_templates")
    torch.cuda.synchronize()
    want = bc.restate_place_templates(bank, first, rows, place, bm_offs, op_rows, op_offs, out_ld)
    return out.cpu().numpy().reshape(n_out + 3, out_ld), want


def check_placements(bank, per_scene, ops, what, lds=(3, 4)):
    for out_ld in lds:
        for misalign in ((False, True) if out_ld == 4 else (False,)):
            got, want = run_placements(bank, per_scene, ops, out_ld, misalign)
            n = want.shape[0]
            _same(got[:n], want, (what, out_ld, misalign))
            assert np.isnan(got[n:]).all(), (what, out_ld, "rows past n_out were written")
    return want


@pytest.mark.parametrize("rows", [0, 1, 255, 256, 257])
def test_one_template_sizes(rows):
    rng = np.random.default_rng(100 + rows)
    bank = rng.uniform(-2, 2, (300, 3)).astype(np.float32)
    want = check_placements(bank, [[(20, rows, _place(rng))]], [_ops(rows)], rows)
    assert want.shape[0] == rows


def test_rotation_form_follows_the_scene_total():
    """two scenes of 44 and 45 rows (templates of 40 + 4 and 40 + 5), same op program but for the flag: the rounded chain against the
    fma form; the restated 44-row scene differs from what the other form would give (the flag is not decoration)"""
    rng = np.random.default_rng(3)
    bank = rng.uniform(-2, 2, (64, 3)).astype(np.float32)
    pl = [_place(rng) for _ in range(4)]
    scenes = [[(0, 40, pl[0]), (40, 4, pl[1])], [(0, 40, pl[2]), (40, 5, pl[3])]]
    ops = [_ops(44, flip=False, scale=None, angle=0.61), _ops(45, flip=False, scale=None, angle=0.61)]
    assert ops[0][0][3] == 1.0 and ops[1][0][3] == 0.0
    want = check_placements(bank, scenes, ops, "44 | 45")
    other = bc.restate_place_templates(bank, [0, 40], [40, 4], np.array(pl[:2], np.float32), [0, 2], np.array(ops[1], np.float32), [0, 1])
    assert other.tobytes() != want[:44].tobytes()


def test_boundaries_inside_a_workgroup():
    """scenes of 100, 0 and 203 rows: workgroup 0 holds two placement boundaries, the empty scene and the scene boundary, workgroup 1 a
    placement boundary; the template of rows 5..64 is placed twice (two scenes, two boxes); per-scene programs differ; the last scene has none"""
    rng = np.random.default_rng(4)
    bank = rng.uniform(-2, 2, (200, 3)).astype(np.float32)
    bank[7] = [-0.0, 0.0, -0.0]
    bank[8] = [0.0, -0.0, -0.0]
    scenes = [[(5, 60, _place(rng, 0.0)), (100, 40, _place(rng))], [], [(5, 60, _place(rng, np.pi / 2)), (0, 143, _place(rng))]]
    ops = [_ops(100, order="rsf"), _ops(0), []]
    want = check_placements(bank, scenes, ops, "boundaries")
    assert want.shape[0] == 303
    # x = -0, y = +0 at yaw 0: (0 + -0) + -0 = +0 before the centre is added; the restatement is what np.einsum gives (test_best_match_cpu)
    zero_centre = [(7, 2, [1.0, -0.0, 0.0, 0.0, -0.0, -0.0, 0.0, 0.0])]
    z = check_placements(bank, [zero_centre], [[]], "signed zeros")
    assert not np.signbit(z[:, 0]).any() and np.signbit(z[0, 2]) == np.signbit(np.float32(-0.0) + np.float32(0.0))


def test_more_placements_than_a_workgroup_stages():
    """150 one-row templates with empty ones between them, then a long one: workgroup 0 spans more placements than it holds in LDS"""
    rng = np.random.default_rng(5)
    bank = rng.uniform(-2, 2, (400, 3)).astype(np.float32)
    a = [(int(rng.integers(0, 400)), k % 3 != 2, _place(rng)) for k in range(225)]       # rows 1, 1, 0, 1, 1, 0, ...
    a = [(f, int(r), p) for f, r, p in a]
    assert sum(r for _, r, _ in a) == 150
    scenes = [a[:100], a[100:] + [(10, 300, _place(rng))]]
    check_placements(bank, scenes, [_ops(70), _ops(400, order="sr")], "staging")


def test_rows_outside_the_bank_are_zeros():
    rng = np.random.default_rng(6)
    bank = rng.uniform(-2, 2, (50, 3)).astype(np.float32)
    scenes = [[(40, 30, _place(rng)), (-5, 10, _place(rng)), (2 ** 31 - 8, 16, _place(rng)), (0, 50, _place(rng))]]
    for out_ld in (3, 4):
        got, want = run_placements(bank, scenes, [_ops(106)], out_ld)
        _same(got[:106], want, ("outside", out_ld))
        xyz = got[:106, out_ld - 3:]
        assert not xyz[10:56].any() and not np.signbit(xyz[10:56]).any() and xyz[:10].all() and xyz[56:].all()


# --------------------------------------------------------------------------------------------------------- fallback, no read-back
def test_a_float64_scene_falls_back_inside_a_batch(tmp_path):
    from btcdet_amd.device_augmentor import DeviceAugmentor, TemplateBank
    scenes = bc.scenes()
    scenes[1]["gt_boxes"] = scenes[1]["gt_boxes"].astype(np.float64)
    aug0, bank0, _, _ = bc.build(tmp_path, "model")
    np.random.seed(ac.SEED)
    pts, offs = _resident(scenes)
    host_dev = DeviceAugmentor(aug0, bank0)
    want_t, want_so = host_dev.apply(pts, offs, host_dev.plan(scenes))["special"]["bm_points"]      # today's route: host, upload
    aug, bank, arrays, _ = bc.build(tmp_path, "model")
    dev_aug = DeviceAugmentor(aug, bank, TemplateBank.from_arrays(arrays))
    np.random.seed(ac.SEED)
    scenes = bc.scenes()                                                # (fresh arrays: a plan may flip a scene's own boxes in place)
    scenes[1]["gt_boxes"] = scenes[1]["gt_boxes"].astype(np.float64)
    plan = dev_aug.plan(scenes)
    assert plan.bm_device == [True, False, True]
    res = dev_aug.apply(pts, offs, plan, indexed_bm=True)
    t, so = res["special"]["bm_points"]
    assert so.tolist() == want_so.tolist() and all(so[b + 1] > so[b] for b in range(3))
    _same(t.cpu().numpy(), want_t.cpu().numpy(), "mixed batch")
    idx = res["bm_points"].cpu().numpy()
    _same(idx[:, 1:], want_t.cpu().numpy(), "mixed batch, indexed")
    assert idx[:, 0].tolist() == np.repeat(np.arange(3, dtype=np.float32), np.diff(so)).tolist()


def test_apply_without_a_read_back(tmp_path):
    from btcdet_amd.device_augmentor import DeviceAugmentor, TemplateBank
    g = golden()
    aug, bank, arrays, _ = bc.build(tmp_path, "model")
    tb = TemplateBank.from_arrays(arrays)
    dev_aug = DeviceAugmentor(aug, bank, tb)
    scenes = bc.scenes()
    pts, offs = _resident(scenes)
    warm_aug, warm_bank, _, _ = bc.build(tmp_path, "model")           # (its own sampler: a plan moves the sampler's cursor)
    warm = DeviceAugmentor(warm_aug, warm_bank, tb)
    warm.apply(pts, offs, warm.plan(scenes), indexed_bm=True)           # (first call: library load, allocator growth, the banks' uploads)
    bank.tensor(DEV)                                                    # (the object bank's one upload)
    np.random.seed(ac.SEED)
    plan = dev_aug.plan(scenes)
    probe = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.sum().item()               # the mode does flag a read-back on this build
        res = dev_aug.apply(pts, offs, plan, sync=False, indexed_bm=True)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    t, so = res["special"]["bm_points"]
    assert "scene_counts" not in res and isinstance(so, np.ndarray)
    for b in range(3):
        _same(t[so[b]:so[b + 1]].cpu().numpy(), g["model%d_bm_points" % b], ("sync=False", b))
    assert res["bm_points"][:, 0].cpu().tolist() == np.repeat(np.arange(3, dtype=np.float32), np.diff(so)).tolist()
