"""CPU-side checks of the augmentation feature (no GPU is touched): btcdet_amd.device_augmentor.DataAugmentor.forward equals, bit for
bit, what the reference's own DataAugmentor.forward wrote (tests/golden/gen_augment_golden.py -> augment.npz) for both shipped queue
orders and both removal widths; DeviceAugmentor.plan leaves the global numpy RNG and every host key where the host chain leaves them,
and its plan -- run through a numpy restatement of the kernels' specification (augment_cases.restate_scene) -- gives the host chain's
points; ObjectBank rows equal the files; the ctypes table matches include/btcdet_hip_augment.h; bad arguments are refused before any launch.

The one GPU primitive on the host path, the BEV IoU inside the sampler, is served by the C oracle's restatement as in
tests/golden/gen_sampler_golden.py (the sampler only asks whether an overlap is zero)."""
import os
import re

import numpy as np
import pytest

import augment_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def host_iou(monkeypatch):
    from btcdet_amd import iou3d_nms
    monkeypatch.setattr(iou3d_nms, "boxes_bev_iou_cpu", ac.oracle_bev_iou)


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "augment.npz"))


@pytest.mark.parametrize("variant", list(ac.VARIANTS))
def test_forward_equals_the_reference(tmp_path, host_iou, variant):
    g = golden()
    aug, _ = ac.build(tmp_path, variant)
    np.random.seed(ac.SEED)
    for i, sc in enumerate(ac.scenes()):
        r = aug.forward(sc)
        ac.check(g, "%s%d_" % (variant, i), r, what=(variant, i))
    assert np.random.random() == float(g[variant + "_rng_next"])


@pytest.mark.parametrize("variant", list(ac.VARIANTS))
def test_plan_equals_the_host_chain(tmp_path, host_iou, variant):
    """same RNG state afterwards, same host keys, and the plan's point work (restated in numpy) gives the recorded points"""
    from btcdet_amd.device_augmentor import DeviceAugmentor
    g = golden()
    aug, bank = ac.build(tmp_path, variant)
    dev = DeviceAugmentor(aug, bank)
    scenes = ac.scenes()
    np.random.seed(ac.SEED)
    plan = dev.plan([{k: v for k, v in s.items() if k != "points"} for s in scenes])     # it is handed no scan
    assert np.random.random() == float(g[variant + "_rng_next"])
    assert plan.batch == 3 and plan.save_pre_rot == (ac.VARIANTS[variant][0] == "model")
    assert plan.rm_boxes.dtype == np.float32 and plan.obj_shift.dtype == np.float64 and plan.ops.dtype == np.float32
    for i, sc in enumerate(scenes):
        p = "%s%d_" % (variant, i)
        host = dict(plan.scenes[i])
        o0, o1 = plan.op_offsets[i], plan.op_offsets[i + 1]
        assert o1 - o0 <= 8
        j0, j1 = plan.obj_offsets[i], plan.obj_offsets[i + 1]
        objects = [(plan.obj_first[j], plan.obj_rows[j]) + tuple(plan.obj_shift[j]) for j in range(j0, j1)]
        assert j1 - j0 == int(host["augment_box_num"]) == plan.rm_offsets[i + 1] - plan.rm_offsets[i]
        pts, pre = ac.restate_scene(sc["points"], plan.rm_boxes[plan.rm_offsets[i]:plan.rm_offsets[i + 1]], bank.rows, objects, plan.ops[o0:o1])
        host["points"] = pts
        if plan.save_pre_rot:
            host["pre_rot_points"] = pre
        for name, rows in ac.SPECIAL:
            host[name] = ac.restate_ops(sc[name], plan.ops[o0:o1], rows)[0]
        ac.check(g, p, host, what=(variant, i))
        if plan.save_pre_rot:
            assert plan.rot_z[i] == np.float32(g[p + "rot_z"])


def test_plan_does_not_touch_the_sampler(tmp_path, host_iou):
    """plan() borrows the sampler's paste for the length of a call: the host chain on the same augmentor still pastes afterwards"""
    from btcdet_amd.device_augmentor import DeviceAugmentor
    g = golden()
    aug, bank = ac.build(tmp_path, "model_w2")
    np.random.seed(ac.SEED)
    DeviceAugmentor(aug, bank).plan(ac.scenes()[:1])
    assert "_paste" not in aug.data_augmentor_queue[0].__dict__
    aug2, _ = ac.build(tmp_path, "model_w2")
    np.random.seed(ac.SEED)
    ac.check(g, "model_w20_", aug2.forward(ac.scenes()[0]))


def test_object_bank_rows_equal_the_files(tmp_path):
    from btcdet_amd.device_augmentor import ObjectBank
    infos = ac.common.make_gt_database(tmp_path)
    bank = ObjectBank(tmp_path, infos, 4)
    n = 0
    for entries in infos.values():
        for e in entries:
            first, rows = bank.table[e["path"]]
            want = np.fromfile(str(tmp_path / e["path"]), dtype=np.float32).reshape(-1, 4)
            assert rows == want.shape[0] == e["num_points_in_gt"]
            assert bank.rows[first:first + rows].tobytes() == want.tobytes()
            n += rows
    assert bank.rows.shape == (n, 4) and bank.rows.dtype == np.float32 and len(bank.table) == 52


def test_queue_follows_the_configuration(tmp_path):
    from btcdet_amd.device_augmentor import DataAugmentor, DeviceAugmentor, ObjectBank
    infos = ac.common.make_gt_database(tmp_path)
    cfg = ac.augmentor_cfg("dataset_w0")
    assert DataAugmentor(tmp_path, cfg, ac.CLASSES, db_infos=infos).queue_names == ["gt_sampling", "random_world_flip", "random_world_rotation",
                                                                                   "random_world_scaling"]
    cfg["DISABLE_AUG_LIST"] = ["random_world_flip", "gt_sampling"]
    assert DataAugmentor(tmp_path, cfg, ac.CLASSES).queue_names == ["random_world_rotation", "random_world_scaling"]
    assert DataAugmentor(tmp_path, ac.queue_cfgs("model_w0")[1:], ac.CLASSES).queue_names == ["random_world_flip", "random_world_scaling",
                                                                                             "random_world_rotation"]
    with pytest.raises(NotImplementedError, match="random_local_rotation"):
        DataAugmentor(tmp_path, [ac.ED(NAME="random_local_rotation")], ac.CLASSES)
    with pytest.raises(NotImplementedError):
        DataAugmentor(tmp_path, [ac.ED(NAME="random_world_flip", ALONG_AXIS_LIST=["x", "y"])], ac.CLASSES)
    with pytest.raises(NotImplementedError):      # the kernels remove and paste before they transform
        q = ac.queue_cfgs("model_w0")
        late = DataAugmentor(tmp_path, [q[1], q[0]], ac.CLASSES, db_infos=ac.common.make_gt_database(tmp_path))
        DeviceAugmentor(late, ObjectBank(tmp_path, infos, 4))


def test_validation_runs_no_training_step(tmp_path):
    aug, _ = ac.build(tmp_path, "model_w0")
    sc = ac.scenes()[1]
    want = {k: np.array(v, copy=True) for k, v in sc.items()}
    keep = want["gt_boxes_mask"]
    state = np.random.get_state()[1].copy()
    r = aug.forward(sc, validation=True)
    assert np.array_equal(np.random.get_state()[1], state)
    assert np.array_equal(r["points"], want["points"]) and "gt_boxes_mask" not in r and "gt_boxes_inds" not in r
    assert np.array_equal(r["gt_boxes"][:, :6], want["gt_boxes"][keep][:, :6]) and list(r["gt_names"]) == list(want["gt_names"][keep])


# ------------------------------------------------------------------------------------------------------------------- C ABI
def _declared():
    src = open(os.path.join(ROOT, "include", "btcdet_hip_augment.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return src, sorted(set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", src)))


def test_ctypes_table_matches_the_header():
    import ctypes
    from btcdet_amd import _lib
    src, names = _declared()
    assert names == sorted(_lib.AUGMENT_EXPORTED_SYMBOLS) == ["btc_augment_batch", "btc_augment_ws_bytes", "btc_world_transform"]
    L = _lib.lib()
    kinds = {"int": _lib.ci, "long long": ctypes.c_longlong, "size_t": _lib.sz}
    for n in names:
        assert hasattr(L, n)
        res, args = _lib._AUGMENT_SIGS[n]
        m = re.search(r"(size_t|int)\s+%s\s*\(([^)]*)\)" % n, src)
        assert kinds[m.group(1)] is res, n
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args), n
        for p, a in zip(params, args):
            want = _lib.vp if "*" in p else kinds[re.sub(r"\s+\w+$", "", p).replace("const ", "").strip()]
            assert a is want, (n, p)
    from btcdet_amd import device_augmentor as da
    consts = dict(re.findall(r"#define (BTC_AUG_\w+) (\d+)", src))
    assert (da.AUG_FLIP_X, da.AUG_SCALE, da.AUG_ROT, da.AUG_MAX_OPS) == tuple(int(consts[k]) for k in ("BTC_AUG_FLIP_X", "BTC_AUG_SCALE", "BTC_AUG_ROT",
                                                                                                      "BTC_AUG_MAX_OPS"))


P = 0x1000      # a non-null address nobody reads: every call below returns from its argument checks


def _batch(L, points=P, n_rows=100, ld=4, offs=P, batch=2, rm=P, rm_offs=P, bank=P, bank_rows=50, first=P, rows=P, shift=P, obj_offs=P, n_obj=3,
           paste=30, ops=P, op_offs=P, cap=130, out=P, pre=P, out_offs=P, ws=P, ws_bytes=1 << 30):
    return L.btc_augment_batch(points, n_rows, ld, offs, batch, rm, rm_offs, bank, bank_rows, first, rows, shift, obj_offs, n_obj, paste, ops, op_offs,
                               cap, out, pre, out_offs, ws, ws_bytes, None)


def test_augment_batch_argument_checks_return_before_any_launch():
    from btcdet_amd import _lib
    L = _lib.lib()
    assert _batch(L, ld=2) == -1 and b"ld >= 3" in L.btc_last_error()
    assert _batch(L, batch=0) == -1 and b"batch >= 1" in L.btc_last_error()
    for kw in (dict(n_rows=-1), dict(n_obj=-1), dict(paste=-1), dict(bank_rows=-1), dict(cap=-1)):
        assert _batch(L, **kw) == -1 and b"negative count" in L.btc_last_error(), kw
    assert _batch(L, cap=129) == -1 and b"out_capacity" in L.btc_last_error()
    assert _batch(L, n_rows=2 ** 31 - 30, cap=2 ** 31) == -1 and b"31 bits" in L.btc_last_error()
    assert _batch(L, n_obj=0, paste=30) == -1
    for kw in ("points", "offs", "rm_offs", "bank", "first", "rows", "shift", "obj_offs", "op_offs", "out", "out_offs", "ws"):
        assert _batch(L, **{kw: None}) == -1 and b"missing pointer" in L.btc_last_error(), kw
    assert _batch(L, ws_bytes=16) == -1 and b"workspace too small" in L.btc_last_error()
    assert L.btc_augment_ws_bytes(100, 2, 3) >= 100 + 3 * 4 * 2 + 4 * 4
    assert L.btc_augment_ws_bytes(10 ** 6, 2, 3) > L.btc_augment_ws_bytes(100, 2, 3) > 0
    assert L.btc_augment_ws_bytes(-1, 2, 3) == 0 and L.btc_augment_ws_bytes(1, 0, 3) == 0


def test_world_transform_argument_checks_return_before_any_launch():
    from btcdet_amd import _lib
    L = _lib.lib()

    def call(inp=P, n=10, ld=3, offs=P, batch=1, ops=P, op_offs=P, out=P + 4096):
        return L.btc_world_transform(inp, n, ld, offs, batch, ops, op_offs, out, None)
    assert call(ld=2) == -1 and b"ld >= 3" in L.btc_last_error()
    assert call(batch=0) == -1
    assert call(n=-1) == -1 and b"negative count" in L.btc_last_error()
    for kw in ("inp", "offs", "op_offs", "out"):
        assert call(**{kw: None}) == -1 and b"missing pointer" in L.btc_last_error(), kw
    assert call(out=P) == -1 and b"alias" in L.btc_last_error()
    assert call(n=0) == 0          # nothing to do, nothing launched


def test_best_match_step_feeds_the_special_sets(tmp_path, host_iou):
    """add_multi_best_match between the sampler and the world transforms (the model config's order): `bm_points` holds the templates of
    the scene's own boxes (data_side.best_match_points) and of the pasted ones, then gets the scene's flip, scale and rotation; plan()
    hands the untransformed set to the device path together with the op program that transforms it"""
    import pickle
    from btcdet_amd import data_side
    from btcdet_amd.device_augmentor import DataAugmentor, DeviceAugmentor, ObjectBank
    infos = ac.common.make_gt_database(tmp_path)
    roots = {"Car": tmp_path / "bm_car", "Pedestrian": tmp_path / "bm_ped"}
    rng = np.random.default_rng(3)
    for r in roots.values():
        r.mkdir()
    for name, entries in infos.items():
        for e in entries:
            with open(roots[name] / "{}_{}.pkl".format(int(e["image_idx"]), e["gt_idx"]), "wb") as f:      # (the sampler hands the index on as int32)
                pickle.dump(rng.uniform(-2, 2, (20 + e["gt_idx"], 3)).astype(np.float32).reshape(-1), f)
    sc = ac.scenes()[0]
    sc["frame_id"] = "000007"
    for i in range(sc["gt_boxes"].shape[0]):
        with open(roots["Car"] / ("7_%d.pkl" % i), "wb") as f:
            pickle.dump(rng.uniform(-2, 2, (30 + i, 3)).astype(np.float32).reshape(-1), f)
    q = ac.queue_cfgs("model_w0")
    cfgs = [q[0], ac.ED(NAME="add_multi_best_match", NUM_POINT_FEATURES=3)] + q[1:]

    def make():
        return DataAugmentor(tmp_path, cfgs, ac.CLASSES, db_infos=ac.common.make_gt_database(tmp_path), template_root=roots)
    aug = make()
    assert aug.queue_names[1] == "add_multi_best_match"
    np.random.seed(ac.SEED)
    r = aug.forward({k: np.array(v, copy=True) for k, v in sc.items()})
    n_own, n_aug = sc["gt_boxes"].shape[0], int(r["augment_box_num"])
    assert r["bm_points"].shape == (sum(30 + i for i in range(n_own)) + sum(20 + int(g) for g in r["aug_boxes_gt_idx"]), 3) and n_aug > 0
    # without the best-match step the same draws give the same boxes and points: the step consumes no random number
    np.random.seed(ac.SEED)
    plain = DataAugmentor(tmp_path, q, ac.CLASSES, db_infos=ac.common.make_gt_database(tmp_path)).forward({k: np.array(v, copy=True) for k, v in sc.items()})
    assert plain["points"].tobytes() == r["points"].tobytes() and plain["gt_boxes"].tobytes() == r["gt_boxes"].tobytes()
    dev = DeviceAugmentor(make(), ObjectBank(tmp_path, infos, 4))
    np.random.seed(ac.SEED)
    plan = dev.plan([sc])
    raw = plan.special[0]["bm_points"]
    assert raw.dtype == np.float32 and raw.shape == r["bm_points"].shape and "bm_points" not in plan.scenes[0]
    own = data_side.best_match_points(sc["gt_boxes"], sc["gt_names"], np.arange(n_own), "000007", roots, ac.CLASSES)
    assert raw[:own.shape[0]].tobytes() == np.ascontiguousarray(own, dtype=np.float32).tobytes()
    got = ac.restate_ops(raw, plan.ops, raw.shape[0])[0]
    assert got.tobytes() == np.ascontiguousarray(r["bm_points"], dtype=np.float32).tobytes()
