"""Inputs shared by the augmentation golden generator (tests/golden/gen_augment_golden.py) and the tests that consume its vectors
(tests/test_augment_cpu.py, tests/test_hip_augment.py): the three scenes of tests/test_hip_database_sampler.py with two special point
sets each (44 and 45 rows: either side of the size at which rotate_points_along_z changes its arithmetic), and the four variants --
the two shipped queue orders x REMOVE_EXTRA_WIDTH 0 / 0.2.  Imports nothing that needs a GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import common  # noqa: E402

CLASSES = ["Car", "Pedestrian"]
SEED = 99
ROT = [-0.78539816, 0.78539816]
# name -> (queue order, REMOVE_EXTRA_WIDTH): "model" = the model config's order (scale, then rotate with SAVE_PRE_ROT),
# "dataset" = the dataset config's (rotate, then scale; LIMIT_WHOLE_SCENE as shipped there)
VARIANTS = {"model_w0": ("model", 0.0), "model_w2": ("model", 0.2), "dataset_w0": ("dataset", 0.0), "dataset_w2": ("dataset", 0.2)}
FULL = "model_w2"          # the variant whose point arrays the golden file holds in full (the others: SHA-1 of the bytes)
SPECIAL = (("miss_points", 44), ("self_points", 45))
POINT_KEYS = ("points", "pre_rot_points") + tuple(k for k, _ in SPECIAL)


class ED(dict):
    __getattr__ = dict.get
    __setattr__ = dict.__setitem__


def sampler_cfg(order, width):
    return ED(NAME="gt_sampling", PREPARE={"filter_by_min_points": ["Car:5", "Pedestrian:5"], "filter_by_difficulty": [-1]},
              SAMPLE_GROUPS=["Car:15", "Pedestrian:4"], NUM_POINT_FEATURES=4, DATABASE_WITH_FAKELIDAR=False, REMOVE_EXTRA_WIDTH=[width] * 3,
              LIMIT_WHOLE_SCENE=order == "dataset", USE_ROAD_PLANE=False)


def queue_cfgs(variant):
    order, width = VARIANTS[variant]
    flip = ED(NAME="random_world_flip", ALONG_AXIS_LIST=["x"])
    scale = ED(NAME="random_world_scaling", WORLD_SCALE_RANGE=[0.95, 1.05])
    if order == "model":
        return [sampler_cfg(order, width), flip, scale, ED(NAME="random_world_rotation", WORLD_ROT_ANGLE=list(ROT), SAVE_PRE_ROT=True)]
    return [sampler_cfg(order, width), flip, ED(NAME="random_world_rotation", WORLD_ROT_ANGLE=list(ROT)), scale]


def augmentor_cfg(variant):
    return ED(DISABLE_AUG_LIST=["placeholder"], AUG_CONFIG_LIST=queue_cfgs(variant))


def scenes():
    from btcdet_amd import synth
    out = []
    for i, seed in enumerate((31, 32, 33)):
        s = synth.make_scene(seed, az_step=0.8)
        n = s["gt_boxes"].shape[0]
        d = {"points": s["points"].copy(), "gt_boxes": s["gt_boxes"][:, :7].copy(), "gt_names": np.array(["Car"] * n),
             "gt_boxes_mask": np.array([True] * n)}
        for k, (name, rows) in enumerate(SPECIAL):
            u = common._hash01(rows * 3, 900 + 10 * i + k).reshape(rows, 3)
            d[name] = (u * np.array([60.0, 60.0, 3.0], np.float32) + np.array([5.0, -30.0, -2.5], np.float32)).astype(np.float32)
        out.append(d)
    if len(out[1]["gt_boxes"]) > 1:      # one box of the second scene was filtered out upstream
        out[1]["gt_boxes_mask"][0] = False
    return out


def record(gold, prefix, r, full):
    """every output key of one scene's result -> gold (point arrays in full, or their shape and SHA-1)"""
    for k in sorted(r):
        v = r[k]
        if k in POINT_KEYS and not full:
            a = np.ascontiguousarray(v)
            gold[prefix + k + "__shape"], gold[prefix + k + "__sha1"] = np.array(a.shape, np.int64), common.sha1(a)
        elif k == "gt_names":
            gold[prefix + k] = np.array([str(x) for x in v])
        else:
            gold[prefix + k] = np.asarray(v)
    gold[prefix + "__keys"] = np.array(sorted(r))


def check(g, prefix, r, what=""):
    """r equals the recorded scene bit for bit: same keys, same dtypes, same bytes"""
    assert sorted(r) == [str(k) for k in g[prefix + "__keys"]], (what, sorted(r))
    for k in sorted(r):
        v = r[k]
        if prefix + k + "__sha1" in g.files:
            a = np.ascontiguousarray(v)
            assert a.dtype == np.float32 and tuple(a.shape) == tuple(int(x) for x in g[prefix + k + "__shape"]), (what, k, a.shape)
            assert np.array_equal(common.sha1(a), g[prefix + k + "__sha1"]), (what, k)
        elif k == "gt_names":
            assert [str(x) for x in v] == [str(x) for x in g[prefix + k]], (what, k)
        else:
            want = g[prefix + k]
            got = np.asarray(v)
            assert got.dtype == want.dtype and got.shape == want.shape, (what, k, got.dtype, want.dtype, got.shape, want.shape)
            assert got.tobytes() == want.tobytes(), (what, k)


def oracle_bev_iou(a, b):
    """stands in for iou3d_nms.boxes_bev_iou_cpu (a HIP kernel) where no GPU is present: the C oracle's restatement, as
    tests/golden/gen_sampler_golden.py uses it; the sampler only asks whether an overlap is zero"""
    from oracle import oracle as orc
    return orc.boxes_iou_bev(np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32))


def build(tmp_path, variant):
    """-> (DataAugmentor, ObjectBank) over a fresh copy of the synthetic database under tmp_path"""
    from btcdet_amd.device_augmentor import DataAugmentor, ObjectBank
    infos = common.make_gt_database(tmp_path)
    bank = ObjectBank(tmp_path, infos, 4)
    return DataAugmentor(tmp_path, augmentor_cfg(variant), CLASSES, db_infos=infos), bank


def restate_ops(pts, ops, n_set):
    """the op program of include/btcdet_hip_augment.h in numpy, on (n, 3 + C) float32 rows of a set of n_set rows
    -> (points, the points as they stood at the first ROT)"""
    from btcdet_amd.data_side import _fma_f32
    p = np.array(pts, dtype=np.float32, copy=True)
    pre = None
    for kind, a, b, _ in ops:
        if int(kind) == 1:
            p[:, 1] = -p[:, 1]
        elif int(kind) == 2:
            p[:, :3] *= np.float32(a)
        elif int(kind) == 3:
            if pre is None:
                pre = p.copy()
            c, s, zero, one = np.float32(a), np.float32(b), np.float32(0), np.float32(1)
            R = [[c, s, zero], [-s, c, zero], [zero, zero, one]]
            x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
            for j in range(3):
                if n_set < 45:
                    p[:, j] = ((np.float32(0) + x * R[0][j]) + y * R[1][j]) + z * R[2][j]
                else:
                    p[:, j] = _fma_f32(z, np.full_like(z, R[2][j]), _fma_f32(y, np.full_like(y, R[1][j]), x * R[0][j]))
    return p, (p.copy() if pre is None else pre)


def restate_scene(scan, rm_rows, bank_rows, objects, ops):
    """btc_augment_batch for one scene in numpy: scan (N, F); rm_rows (R, 8); objects = [(first, n, cx, cy, cz, lift)]; ops (k, 4)"""
    x, y, z = scan[:, 0], scan[:, 1], scan[:, 2]
    removed = np.zeros(scan.shape[0], bool)
    for b in np.asarray(rm_rows, np.float32):
        sx, sy = x - b[0], y - b[1]
        lx, ly = sx * b[6] - sy * b[7], sx * b[7] + sy * b[6]
        removed |= (np.abs(z - b[2]) <= b[5]) & (np.abs(lx) < b[3]) & (np.abs(ly) < b[4])
    parts = [scan[~removed]]
    for first, n, cx, cy, cz, lift in objects:
        o = bank_rows[int(first):int(first) + int(n)].copy()
        o[:, :3] = (o[:, :3].astype(np.float64) + np.array([cx, cy, cz], np.float64)).astype(np.float32)
        o[:, 2] = (o[:, 2].astype(np.float64) - np.float64(lift)).astype(np.float32)
        parts.append(o)
    allp = np.concatenate(parts, axis=0)
    return restate_ops(allp, ops, allp.shape[0])
