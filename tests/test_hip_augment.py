"""The augmentation of a resident batch (btcdet_amd.device_augmentor.DeviceAugmentor, csrc/augment.hip) against the host chain,
DataAugmentor.forward per scene from the same seed -- itself pinned to the reference's own class by tests/test_augment_cpu.py.  The
expectation is never the device code.  Everything is compared EXACTLY (bytes): every input of the point-in-box test is formed on the
host, and the device arithmetic is spelled out unfused.

  whole path   the three scenes as one batch and as three batches of one, both queue orders, both removal widths: points,
               pre_rot_points, rot_z, scene_offsets, every host key, two special sets per scene (44 and 45 rows)
  edge shapes  hand-made plans through btc_augment_batch; expectation = database_sampler.points_in_boxes_mask + the host functions
               (scene sizes around a workgroup, boundaries inside one, 63 / 64 / 65 / 129 pasted objects around the 64 of a wave)
  sync=False   under torch.cuda.set_sync_debug_mode("error")
  chained      DataProcessor.forward_raw_batch on apply's output == on the uploaded host-chain result, same shuffle_idx"""
import numpy as np
import pytest
import torch

import augment_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(got.shape[0], -1).any(axis=1))[0]
        raise AssertionError("%s: %d of %d rows differ, first %d: got %s want %s" % (what, bad.size, got.shape[0], bad[0], got[bad[0]], want[bad[0]]))


_HOST = {}


def host_chain(tmp_path_factory, variant):
    """DataAugmentor.forward over the three scenes from the seed, computed once per variant and left unchanged"""
    if variant not in _HOST:
        aug, _ = ac.build(tmp_path_factory.mktemp("host_" + variant), variant)
        np.random.seed(ac.SEED)
        res = [aug.forward(sc) for sc in ac.scenes()]
        _HOST[variant] = (res, np.random.random())
    return _HOST[variant]


def device_run(dev_aug, scenes, sync=True):
    pts = torch.from_numpy(np.concatenate([s["points"] for s in scenes])).to(DEV)
    offs = torch.from_numpy(np.cumsum([0] + [s["points"].shape[0] for s in scenes]).astype(np.int32)).to(DEV)
    special = {name: (torch.from_numpy(np.concatenate([s[name] for s in scenes])).to(DEV), np.cumsum([0] + [s[name].shape[0] for s in scenes]))
               for name, _ in ac.SPECIAL}
    plan = dev_aug.plan(scenes)
    return dev_aug.apply(pts, offs, plan, special=special, sync=sync), plan


def compare_scene(res, b, want, what):
    """scene b of an apply result == one DataAugmentor.forward result, every key"""
    bounds = res["scene_offsets"].cpu().numpy()
    assert bounds.dtype == np.int32
    keys = set(want)
    _same(res["points"][bounds[b]:bounds[b + 1]].cpu().numpy(), want["points"], (what, "points"))
    keys -= {"points"}
    if "pre_rot_points" in want:
        _same(res["pre_rot_points"][bounds[b]:bounds[b + 1]].cpu().numpy(), want["pre_rot_points"], (what, "pre_rot_points"))
        rot = res["rot_z"].cpu().numpy()
        assert rot.dtype == np.float32 and rot[b] == np.float32(want["rot_z"]), (what, rot[b], want["rot_z"])
        keys -= {"pre_rot_points", "rot_z"}
    else:
        assert "pre_rot_points" not in res and "rot_z" not in res
    for name, _ in ac.SPECIAL:
        t, so = res["special"][name]
        _same(t[so[b]:so[b + 1]].cpu().numpy(), want[name], (what, name))
        keys -= {name}
    for k in sorted(keys):
        got = res[k][b]
        if k == "gt_names":
            assert [str(x) for x in got] == [str(x) for x in want[k]], (what, k)
        else:
            g, w = np.asarray(got), np.asarray(want[k])
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, k)
    assert int(res["scene_counts"][b]) == want["points"].shape[0]


@pytest.mark.parametrize("grouping", ["one_batch", "three_batches"])
@pytest.mark.parametrize("variant", list(ac.VARIANTS))
def test_whole_path_equals_the_host_chain(tmp_path_factory, variant, grouping):
    from btcdet_amd.device_augmentor import DeviceAugmentor
    want, rng_next = host_chain(tmp_path_factory, variant)
    aug, bank = ac.build(tmp_path_factory.mktemp("dev"), variant)
    dev_aug = DeviceAugmentor(aug, bank)
    scenes = ac.scenes()
    groups = [scenes] if grouping == "one_batch" else [[s] for s in scenes]
    np.random.seed(ac.SEED)
    i = 0
    for grp in groups:
        res, plan = device_run(dev_aug, grp)
        assert res["scene_offsets"].is_cuda and int(res["scene_offsets"][-1]) == res["points"].shape[0]
        for b in range(len(grp)):
            compare_scene(res, b, want[i], (variant, grouping, i))
            i += 1
    assert np.random.random() == rng_next


# ------------------------------------------------------------------------------------------------- edge shapes through the C ABI
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cos_sin(angle):
    """as data_side.rotate_points_along_z forms them"""
    a = torch.from_numpy(np.array([angle])).float()
    return float(torch.cos(a)[0]), float(torch.sin(a)[0])


def raw_augment(scans, boxes, objects, bank, ops, ld, with_pre=True):
    """btc_augment_batch with a hand-made plan.  scans: list of (N_b, ld); boxes: list of (R_b, 7); objects: list of lists of
    (first, n, centre xyz (float64), lift); ops: list of lists of (kind, a, b) -> (out, out_pre or None, out_offsets) as numpy"""
    from btcdet_amd._lib import check, ptr, stream_ptr
    from btcdet_amd.device_augmentor import removal_rows
    B = len(scans)
    pts = np.concatenate(scans).astype(np.float32).reshape(-1, ld)
    n = pts.shape[0]
    offs = np.cumsum([0] + [s.shape[0] for s in scans]).astype(np.int32)
    rm = np.concatenate([removal_rows(np.asarray(b, np.float32).reshape(-1, 7)) for b in boxes]).astype(np.float32).reshape(-1, 8)
    rm_offs = np.cumsum([0] + [len(b) for b in boxes]).astype(np.int32)
    flat = [o for per in objects for o in per]
    first = np.array([o[0] for o in flat], np.int32)
    rows = np.array([o[1] for o in flat], np.int32)
    shift = np.array([list(o[2]) + [o[3]] for o in flat], np.float64).reshape(-1, 4)
    obj_offs = np.cumsum([0] + [len(per) for per in objects]).astype(np.int32)
    op_rows = np.array([list(o) + [0.0] * (4 - len(o)) for per in ops for o in per], np.float32).reshape(-1, 4)
    op_offs = np.cumsum([0] + [len(per) for per in ops]).astype(np.int32)
    paste = int(rows.sum())
    cap = n + paste
    d = dict(pts=_t(pts) if n else None, offs=_t(offs), rm=_t(rm) if rm.size else None, rm_offs=_t(rm_offs), bank=_t(bank), first=_t(first) if flat else None,
             rows=_t(rows) if flat else None, shift=_t(shift) if flat else None, obj_offs=_t(obj_offs), ops=_t(op_rows) if op_rows.size else None,
             op_offs=_t(op_offs))
    out = torch.full((max(cap, 1), ld), float("nan"), device=DEV)
    pre = torch.full((max(cap, 1), ld), float("nan"), device=DEV) if with_pre else None
    new_offs = torch.full((B + 1,), -7, dtype=torch.int32, device=DEV)
    ws_bytes = L().btc_augment_ws_bytes(n, B, len(flat))
    ws = torch.empty((max(ws_bytes, 256),), dtype=torch.uint8, device=DEV)
    check(L().btc_augment_batch(ptr(d["pts"]), n, ld, ptr(d["offs"]), B, ptr(d["rm"]), ptr(d["rm_offs"]), ptr(d["bank"]), bank.shape[0], ptr(d["first"]),
                                ptr(d["rows"]), ptr(d["shift"]), ptr(d["obj_offs"]), len(flat), paste, ptr(d["ops"]), ptr(d["op_offs"]), cap, ptr(out),
                                ptr(pre), ptr(new_offs), ptr(ws), ws_bytes, stream_ptr()), "btc_augment_batch")
    torch.cuda.synchronize()
    return out.cpu().numpy(), (pre.cpu().numpy() if with_pre else None), new_offs.cpu().numpy()


def host_expect(scan, boxes, objects, bank, ops):
    """one scene by the host functions: points_in_boxes_mask, the paste of DataBaseSampler._paste, data_side's transforms"""
    from btcdet_amd import data_side
    from btcdet_amd.database_sampler import points_in_boxes_mask
    boxes = np.asarray(boxes, np.float32).reshape(-1, 7)
    keep = ~points_in_boxes_mask(scan[:, 0:3], boxes).any(axis=0) if boxes.shape[0] else np.ones(scan.shape[0], bool)
    clouds = []
    for first, n, centre, lift in objects:
        obj = bank[first:first + n].copy()
        obj[:, :3] += np.asarray(centre, np.float64)
        obj[:, 2] -= np.float64(lift)
        clouds.append(obj)
    pts = np.concatenate([scan[keep]] + clouds, axis=0)
    pre = None
    dummy = np.zeros((0, 7), np.float32)
    for op in ops:
        if op[0] == 1:
            _, pts, _ = data_side.random_flip_along_x(dummy, pts, enable=True)
        elif op[0] == 2:
            pts[:, :3] *= float(op[3])                  # global_scaling's expression with its Python float
        else:
            if pre is None:
                pre = pts
            pts = data_side.rotate_points_along_z(pts[np.newaxis, :, :], np.array([op[3]]))[0]
    return pts, (pts if pre is None else pre), int(keep.sum())


def _ops(flip=True, scale=1.03125, angle=0.3, order="fsr"):
    """(device ops, host ops): the host side keeps the Python float of the scale and the angle itself"""
    dev, host = [], []
    for ch in order:
        if ch == "f" and flip:
            dev.append((1,)), host.append((1, 0, 0, None))
        elif ch == "s" and scale is not None:
            dev.append((2, np.float32(scale))), host.append((2, 0, 0, scale))
        elif ch == "r" and angle is not None:
            c, s = _cos_sin(angle)
            dev.append((3, c, s)), host.append((3, 0, 0, angle))
    return dev, host


def _scene(rng, n, ld, lo=(0, -20, -2), hi=(40, 20, 1)):
    p = rng.uniform(-1, 1, (n, ld)).astype(np.float32)
    p[:, :3] = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    return p


def _bank(rng, ld, rows=40):
    return rng.uniform(-1.5, 1.5, (rows, ld)).astype(np.float32)


def _boxes(rng, r, centre=(20, 0, -0.5)):
    """r boxes scattered over the scan's range, big enough to remove some points each"""
    c = rng.uniform((2, -18, -1), (38, 18, 0), (r, 3))
    c[0:1] = centre
    return np.concatenate([c, rng.uniform((3, 1.5, 1.5), (8, 6, 3), (r, 3)), rng.uniform(-3.1, 3.1, (r, 1))], axis=1).astype(np.float32)


def check_case(scans, boxes, objects, bank, ops_dev, ops_host, ld, with_pre=True, expect_kept=None):
    out, pre, offs = raw_augment(scans, boxes, objects, bank, ops_dev, ld, with_pre)
    assert offs[0] == 0
    total = 0
    for b in range(len(scans)):
        want, want_pre, kept = host_expect(scans[b], boxes[b], objects[b], bank, ops_host[b])
        if expect_kept is not None:
            assert kept == expect_kept[b], (b, kept)
        assert offs[b + 1] - offs[b] == want.shape[0], (b, offs, want.shape)
        _same(out[offs[b]:offs[b + 1]], want, ("out", b))
        if with_pre:
            _same(pre[offs[b]:offs[b + 1]], want_pre, ("out_pre", b))
        total += want.shape[0]
    assert offs[-1] == total
    assert np.isnan(out[total:]).all(), "rows past the total were written"


@pytest.mark.parametrize("ld", [3, 4, 5])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_one_scene_sizes_and_row_widths(n, ld):
    rng = np.random.default_rng(1000 + 10 * n + ld)
    bank = _bank(rng, ld)
    dev, host = _ops()
    boxes = _boxes(rng, 1) if n else np.zeros((0, 7), np.float32)
    if n == 1:
        boxes[0, :3] = (100, 100, 0)           # the only row stays
    objects = [(3, 7, (10.25, -3.5, -0.75), 0.125), (11, 1, (30.0, 5.0, -1.0), 0.0)]     # the second: a one-point object
    check_case([_scene(rng, n, ld)], [boxes], [objects], bank, [dev], [host], ld)


def test_uneven_batch_with_a_scene_boundary_inside_a_workgroup():
    """scenes of 100, 257 and 3 rows: workgroup 0 holds the first boundary, workgroup 1 the second; removal boxes 64 / 65 / 0 (one LDS
    chunk, two, none); the middle scene gets nothing pasted; per-scene op programs differ (rotation first / none / scale after rotation)"""
    rng = np.random.default_rng(7)
    ld = 4
    bank = _bank(rng, ld)
    scans = [_scene(rng, 100, ld), _scene(rng, 257, ld), _scene(rng, 3, ld)]
    boxes = [_boxes(rng, 64), _boxes(rng, 65), np.zeros((0, 7), np.float32)]
    objects = [[(0, 5, (1.5, 2.5, -1.0), 0.0), (20, 20, (33.0, -7.0, -0.5), 0.25)], [], [(39, 1, (5.0, 5.0, 0.0), 0.0)]]
    d0, h0 = _ops(order="rsf")
    d1, h1 = _ops(angle=None)                   # no ROT: out_pre equals out
    d2, h2 = _ops(flip=False, order="rs", angle=-0.7)
    check_case(scans, boxes, objects, bank, [d0, d1, d2], [h0, h1, h2], ld)
    check_case(scans, boxes, objects, bank, [d0, d1, d2], [h0, h1, h2], ld, with_pre=False)


@pytest.mark.parametrize("n_objects", [63, 64, 65, 129])
def test_pasted_objects_around_the_chunks_of_the_object_scan(n_objects):
    """one wave scans the objects' row counts 64 at a time, and one wave per scene boundary sums the rows pasted in front of it 64
    objects at a time: objects of 1 - 3 rows, all but four in the first scene, none in the second, the last four in the third"""
    rng = np.random.default_rng(300 + n_objects)
    ld = 4
    bank = _bank(rng, ld)
    scans = [_scene(rng, 70, ld), _scene(rng, 30, ld), _scene(rng, 5, ld)]
    boxes = [_boxes(rng, 1), np.zeros((0, 7), np.float32), _boxes(rng, 1)]
    rows = rng.integers(1, 4, n_objects)
    objs = [(int(rng.integers(0, bank.shape[0] - 3)), int(r), tuple(rng.uniform((0, -20, -2), (40, 20, 1))), float(rng.integers(0, 3)) / 8) for r in rows]
    objects = [objs[:-4], [], objs[-4:]]
    d0, h0 = _ops()
    d2, h2 = _ops(flip=False, order="rs", angle=-0.7)
    check_case(scans, boxes, objects, bank, [d0, [], d2], [h0, [], h2], ld)


def test_every_row_removed_and_empty_programs():
    rng = np.random.default_rng(8)
    ld = 4
    bank = _bank(rng, ld)
    scans = [_scene(rng, 300, ld), _scene(rng, 40, ld), _scene(rng, 0, ld)]
    everything = np.array([[20, 0, -0.5, 100, 100, 10, 0.4]], np.float32)
    boxes = [everything, np.zeros((0, 7), np.float32), everything]
    objects = [[], [], []]
    d, h = _ops()
    check_case(scans, boxes, objects, bank, [d, [], []], [h, [], []], ld, expect_kept=[0, 40, 0])
    objects = [[(2, 3, (1.0, 1.0, 1.0), 0.0)], [], []]          # a scene that consists of its pasted rows alone
    check_case(scans, boxes, objects, bank, [d, [], d], [h, [], h], ld, expect_kept=[0, 40, 0])


@pytest.mark.parametrize("pasted", [0, 1])
def test_rotation_form_follows_the_emitted_row_count(pasted):
    """50 rows of which 6 sit in the removal box: 44 rows are left (the rounded chain); with a one-point object 45 (the fma form).  The
    host function chooses by the array it is handed; the kernel must choose by the count it finds"""
    rng = np.random.default_rng(9)
    ld = 4
    bank = _bank(rng, ld)
    scan = _scene(rng, 50, ld, lo=(0, -20, -2), hi=(10, 20, 1))
    scan[10:16, :3] = rng.uniform((29, -0.5, -0.9), (31, 0.5, -0.1), (6, 3)).astype(np.float32)
    boxes = np.array([[30, 0, -0.5, 4, 2, 1.5, 0.2]], np.float32)
    objects = [(5, 1, (12.0, 3.0, -1.0), 0.0)] if pasted else []
    d, h = _ops(flip=False, scale=None, angle=0.61)
    check_case([scan], [boxes], [objects], bank, [d], [h], ld, expect_kept=[44])


def test_points_on_the_faces():
    """heading 0, dyadic coordinates, box centred at the origin in x and y so that every difference is exact: a point exactly on a z
    face is inside (<=) and removed; a point exactly at hx = dx/2 + margin is outside (strict) and stays, its neighbour below goes"""
    from btcdet_amd.database_sampler import points_in_boxes_mask
    box = np.array([[0, 0, 1, 4, 2, 2, 0]], np.float32)
    hx = np.float32(4) / np.float32(2.0) + np.float32(1e-2)
    hy = np.float32(2) / np.float32(2.0) + np.float32(1e-2)
    below = lambda v: np.nextafter(np.float32(v), np.float32(0))
    above = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))
    pts = np.array([[0.5, 0.25, 2.0, 0.1],                # on the upper z face: removed
                    [0.5, 0.25, 0.0, 0.2],                # on the lower z face: removed
                    [0.5, 0.25, above(2.0), 0.3],         # just above: stays
                    [hx, 0.25, 1.0, 0.4],                 # exactly at hx: stays
                    [-hx, 0.25, 1.0, 0.5],
                    [below(hx), 0.25, 1.0, 0.6],          # just inside: removed
                    [0.5, hy, 1.0, 0.7],                  # exactly at hy: stays
                    [0.5, -below(hy), 1.0, 0.8],          # just inside: removed
                    [0.5, 0.25, float("nan"), 0.9]], np.float32)       # NaN compares false: stays
    want_keep = np.array([False, False, True, True, True, False, True, False, True])
    assert np.array_equal(~points_in_boxes_mask(pts[:, :3], box).any(axis=0), want_keep)
    out, pre, offs = raw_augment([pts], [box], [[]], np.zeros((1, 4), np.float32), [[]], 4)
    assert offs.tolist() == [0, int(want_keep.sum())]
    _same(out[:offs[1]], pts[want_keep], "faces")
    _same(pre[:offs[1]], pts[want_keep], "faces pre")


# --------------------------------------------------------------------------------------------------------- no read-back, chained
def test_apply_without_a_read_back(tmp_path_factory):
    from btcdet_amd.device_augmentor import DeviceAugmentor
    variant = "model_w2"
    want, _ = host_chain(tmp_path_factory, variant)
    aug, bank = ac.build(tmp_path_factory.mktemp("dev"), variant)
    dev_aug = DeviceAugmentor(aug, bank)
    scenes = ac.scenes()
    warm_aug, warm_bank = ac.build(tmp_path_factory.mktemp("warm"), variant)      # (its own sampler: a plan moves the sampler's cursor)
    device_run(DeviceAugmentor(warm_aug, warm_bank), scenes[:1])                  # (first call: library load, allocator growth)
    bank.tensor(DEV)                                                              # (the bank's one upload)
    np.random.seed(ac.SEED)
    pts = torch.from_numpy(np.concatenate([s["points"] for s in scenes])).to(DEV)
    offs = torch.from_numpy(np.cumsum([0] + [s["points"].shape[0] for s in scenes]).astype(np.int32)).to(DEV)
    special = {name: (torch.from_numpy(np.concatenate([s[name] for s in scenes])).to(DEV), np.cumsum([0] + [s[name].shape[0] for s in scenes]))
               for name, _ in ac.SPECIAL}
    plan = dev_aug.plan(scenes)              # (host work; the sampler's IoU kernel reads its result back)
    probe = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.sum().item()               # the mode does flag a read-back on this build
        res = dev_aug.apply(pts, offs, plan, special=special, sync=False)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    assert "scene_counts" not in res and res["points"].shape[0] == pts.shape[0] + plan.paste_rows == res["pre_rot_points"].shape[0]
    res["scene_counts"] = [w["points"].shape[0] for w in want]
    for b in range(3):
        compare_scene(res, b, want[b], ("sync=False", b))


def test_forward_raw_batch_on_the_device_result(tmp_path_factory):
    """the resident pipeline from the raw scan: forward_raw_batch(apply(...)) gives the six voxel tensors of forward_raw_batch on the
    uploaded host-chain result, with the same shuffle_idx"""
    from btcdet_amd.config import load_cfg
    from btcdet_amd.device_augmentor import DeviceAugmentor
    from btcdet_amd.processor import DataProcessor
    variant = "model_w0"
    want, _ = host_chain(tmp_path_factory, variant)
    d = load_cfg().DATA_CONFIG
    proc = DataProcessor(d.DATA_PROCESSOR, point_cloud_range=np.array(d.OCC.POINT_CLOUD_RANGE, dtype=np.float32), training=True, occ_config=d.OCC,
                         det_point_cloud_range=np.array(d.POINT_CLOUD_RANGE, dtype=np.float32))
    h_pts = torch.from_numpy(np.concatenate([w["points"] for w in want])).to(DEV)
    h_pre = torch.from_numpy(np.concatenate([w["pre_rot_points"] for w in want])).to(DEV)
    h_offs = torch.from_numpy(np.cumsum([0] + [w["points"].shape[0] for w in want]).astype(np.int32)).to(DEV)
    h_rot = torch.tensor([w["rot_z"] for w in want], dtype=torch.float32, device=DEV)
    flag = getattr(proc, "_shuffle_flag", None)      # the permutations need the masked counts: one masking pass without the shuffle tells them
    proc._shuffle_flag = False
    _, _, _, counts = proc.mask_and_shuffle_batch(h_pts, h_pre, h_offs)
    proc._shuffle_flag = flag
    assert proc._shuffle_enabled(), "the training configuration shuffles"
    perms = [np.random.default_rng(5 + b).permutation(c) for b, c in enumerate(counts)]
    ref = proc.forward_raw_batch(h_pts, h_pre, h_offs, h_rot, shuffle_idx=perms)
    aug, bank = ac.build(tmp_path_factory.mktemp("dev"), variant)
    np.random.seed(ac.SEED)
    res, _ = device_run(DeviceAugmentor(aug, bank), ac.scenes())
    got = proc.forward_raw_batch(res["points"], res["pre_rot_points"], res["scene_offsets"], res["rot_z"], shuffle_idx=perms)
    assert got["scene_counts"] == ref["scene_counts"] == counts
    for k in ("voxels", "voxel_coords", "voxel_num_points", "det_voxels", "det_voxel_coords", "det_voxel_num_points"):
        assert got[k].shape == ref[k].shape and got[k].shape[0] > 0, k
        assert torch.equal(got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k],
                           ref[k].view(torch.int32) if ref[k].dtype == torch.float32 else ref[k]), k
