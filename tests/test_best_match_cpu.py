"""CPU-side checks of the resident best-match step (no GPU is touched): TemplateBank rows equal the files; the host DataAugmentor's
`bm_points` equal, bit for bit, what the reference's own DataAugmentor.forward with its own MltBestMatchQuerier wrote
(tests/golden/gen_best_match_golden.py -> best_match.npz); DeviceAugmentor.plan with a bank leaves the RNG and every host key where the
host chain leaves them, forms no point, and its placements -- run through the numpy restatement of include/btcdet_hip_bestmatch.h
(best_match_cases.restate_rows) and the op program -- give the recorded bytes; the restatement equals np.einsum itself on signed
zeros and the axis yaws; missing templates raise, float64 boxes take the host route; the ctypes table matches the header; bad
arguments are refused before any launch.  Every comparison is of bytes."""
import ctypes
import os
import re

import numpy as np
import pytest

import augment_cases as ac
import best_match_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def host_iou(monkeypatch):
    from btcdet_amd import iou3d_nms
    monkeypatch.setattr(iou3d_nms, "boxes_bev_iou_cpu", ac.oracle_bev_iou)


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "best_match.npz"))


def _no_scan(scenes):
    return [{k: v for k, v in s.items() if k != "points"} for s in scenes]


def test_template_bank_rows_equal_the_files(tmp_path):
    from btcdet_amd import data_side
    from btcdet_amd.device_augmentor import TemplateBank
    arrays = bc.templates(ac.common.make_gt_database(tmp_path))
    roots = bc.write_templates(tmp_path, arrays)
    (roots["Car"] / "notes.txt").write_text("not a template")
    bank = TemplateBank(dict(roots, Cyclist=tmp_path / "absent"))
    assert sorted(bank.table) == sorted(arrays) and len(arrays) > 52
    n = 0
    for (name, img, gt), (first, rows) in bank.table.items():
        want = data_side.read_bm_template(roots[name] / "{}_{}.pkl".format(img, gt), 3)
        assert rows == want.shape[0] and 20 <= rows <= 60
        assert bank.rows[first:first + rows].tobytes() == want.tobytes() == arrays[(name, img, gt)].tobytes()
        n += rows
    assert bank.rows.shape == (n, 3) and bank.rows.dtype == np.float32 and bank.nbytes == 12 * n
    mem = TemplateBank.from_arrays(arrays)
    assert mem.table == bank.table and mem.rows.tobytes() == bank.rows.tobytes() and mem.nbytes == bank.nbytes
    some = [("Pedestrian", 103, 3), ("Car", 7, 0), ("Car", 7, 0)]
    part = TemplateBank(roots, keys=some)
    assert sorted(part.table) == sorted(set(some)) and part.rows.shape[0] == sum(arrays[k].shape[0] for k in set(some))
    for k in set(some):
        first, rows = part.table[k]
        assert part.rows[first:first + rows].tobytes() == arrays[k].tobytes()
    with pytest.raises(KeyError, match="7_99.pkl"):
        TemplateBank(roots, keys=[("Car", 7, 99)])
    six = {("Car", 1, 0): np.arange(24, dtype=np.float64)}       # LOAD_POINT_FEATURES = 6: the first three columns of every row
    (tmp_path / "six").mkdir()
    bc.pickle.dump(six[("Car", 1, 0)], open(tmp_path / "six" / "1_0.pkl", "wb"))
    wide = TemplateBank({"Car": tmp_path / "six"}, load_point_features=6)
    assert wide.rows.tolist() == [[0, 1, 2], [6, 7, 8], [12, 13, 14], [18, 19, 20]]


@pytest.mark.parametrize("order", list(bc.ORDERS))
def test_host_forward_equals_the_reference(tmp_path, host_iou, order):
    g = golden()
    aug, _, _, _ = bc.build(tmp_path, order)
    np.random.seed(ac.SEED)
    for i, sc in enumerate(bc.scenes()):
        r = aug.forward(sc)
        assert r["bm_points"].dtype == np.float32 and r["bm_points"].tobytes() == g["%s%d_bm_points" % (order, i)].tobytes()
        ac.check(g, "%s%d_" % (order, i), r, what=(order, i))
    assert np.random.random() == float(g[order + "_rng_next"])


@pytest.mark.parametrize("order", list(bc.ORDERS))
def test_plan_with_a_bank_equals_the_host_chain(tmp_path, host_iou, order):
    """same RNG state and host keys as the plan without a bank and as the reference; no bm_points formed on the host; the placements,
    restated, give the recorded bytes"""
    from btcdet_amd.device_augmentor import DeviceAugmentor, TemplateBank
    g = golden()
    scenes = bc.scenes()
    aug0, bank0, _, _ = bc.build(tmp_path / "a", order)
    np.random.seed(ac.SEED)
    plain = DeviceAugmentor(aug0, bank0).plan(_no_scan(scenes))
    after_plain = np.random.random()
    aug, bank, arrays, roots = bc.build(tmp_path / "b", order)
    tb = TemplateBank(roots)
    dev = DeviceAugmentor(aug, bank, tb)
    np.random.seed(ac.SEED)
    state = np.random.get_state()[1].copy()
    plan = dev.plan(_no_scan(scenes))
    assert not np.array_equal(np.random.get_state()[1], state)              # (the sampler and the world steps drew)
    assert np.random.random() == after_plain == float(g[order + "_rng_next"])
    assert plan.bm_device == [True] * 3 and plain.bm_device == [False] * 3 and plain.bm_rows_total == 0
    want_rows = [g["%s%d_bm_points" % (order, i)].shape[0] for i in range(3)]
    assert plan.bm_rows_total == sum(want_rows) > 0                          # a silent fallback would place nothing
    assert plan.bm_first.dtype == plan.bm_rows.dtype == plan.bm_offsets.dtype == plan.bm_row_offsets.dtype == np.int32
    assert plan.bm_place.dtype == np.float32 and plan.bm_place.shape == (plan.bm_first.shape[0], 8) and not plan.bm_place[:, 6:].any()
    assert plan.bm_row_offsets.tolist() == np.concatenate([[0], np.cumsum(plan.bm_rows)]).tolist()
    assert plan.bm_offsets[0] == 0 and plan.bm_offsets[-1] == plan.bm_first.shape[0]
    assert plan.ops.tobytes() == plain.ops.tobytes() and not plan.ops[:, 3].any()       # >= 45 rows a scene: the fma form
    for i, sc in enumerate(scenes):
        p = "%s%d_" % (order, i)
        assert "bm_points" not in plan.special[i] and "bm_points" not in plan.scenes[i]
        assert plain.special[i]["bm_points"].shape[0] == want_rows[i]
        assert sorted(plan.scenes[i]) == sorted(plain.scenes[i])
        for k, v in plan.scenes[i].items():
            assert np.asarray(v).tobytes() == np.asarray(plain.scenes[i][k]).tobytes(), (i, k)
        j0, j1 = plan.bm_offsets[i], plan.bm_offsets[i + 1]
        n_own = plan.scenes[i]["gt_boxes"].shape[0] - int(plan.scenes[i]["augment_box_num"])
        assert j1 - j0 == plan.scenes[i]["gt_boxes"].shape[0]               # every box is a Car or a Pedestrian: one placement each
        keys = [("Car", int(sc["frame_id"]), int(k)) for k in np.nonzero(sc["gt_boxes_mask"])[0]] + \
               [(str(n), int(a), int(b)) for n, a, b in zip(plan.scenes[i]["gt_names"][n_own:], plan.scenes[i]["aug_boxes_image_idx"],
                                                            plan.scenes[i]["aug_boxes_gt_idx"])]
        assert [(int(f), int(r)) for f, r in zip(plan.bm_first[j0:j1], plan.bm_rows[j0:j1])] == [tb.table[k] for k in keys]
        o0, o1 = plan.op_offsets[i], plan.op_offsets[i + 1]
        got = bc.restate_place_templates(tb.rows, plan.bm_first, plan.bm_rows, plan.bm_place, [j0, j1], plan.ops[o0:o1], [0, o1 - o0])
        assert got.tobytes() == g[p + "bm_points"].tobytes(), (order, i)
        # the whole scene as the reference recorded it: the scan's part restated as tests/test_augment_cpu.py does
        host = dict(plan.scenes[i])
        r0, r1 = plan.obj_offsets[i], plan.obj_offsets[i + 1]
        objects = [(plan.obj_first[j], plan.obj_rows[j]) + tuple(plan.obj_shift[j]) for j in range(r0, r1)]
        pts, pre = ac.restate_scene(sc["points"], plan.rm_boxes[plan.rm_offsets[i]:plan.rm_offsets[i + 1]], bank.rows, objects, plan.ops[o0:o1])
        host["points"], host["bm_points"] = pts, got
        if plan.save_pre_rot:
            host["pre_rot_points"] = pre
        for name, rows in ac.SPECIAL:
            host[name] = ac.restate_ops(sc[name], plan.ops[o0:o1], rows)[0]
        ac.check(g, p, host, what=(order, i))


def test_small_scene_sets_the_rounded_chain_flag(tmp_path, host_iou):
    """a scene whose bm_points stay below 45 rows: its ops carry flag 1 (the rotation form rotate_points_along_z takes for such a set),
    and the restated placements equal the host chain's bm_points"""
    from btcdet_amd.device_augmentor import DataAugmentor, DeviceAugmentor, TemplateBank
    q = bc.queue_cfgs("model")[1:]                                            # no sampler: the scene's own boxes alone
    sc = bc.scenes()[0]
    keep = np.zeros(sc["gt_boxes"].shape[0], bool)
    keep[:1] = True
    sc["gt_boxes"], sc["gt_names"], sc["gt_boxes_mask"] = sc["gt_boxes"][keep], sc["gt_names"][keep], sc["gt_boxes_mask"][keep]
    arrays = {("Car", 7, 0): np.random.default_rng(1).uniform(-2, 2, (44, 3)).astype(np.float32)}
    roots = bc.write_templates(tmp_path, arrays)
    aug = DataAugmentor(tmp_path, q, ac.CLASSES, template_root=roots)
    np.random.seed(5)
    want = aug.forward({k: np.array(v, copy=True) for k, v in sc.items()})["bm_points"]
    np.random.seed(5)
    plan = DeviceAugmentor(aug, None, TemplateBank.from_arrays(arrays)).plan(_no_scan([sc]))
    assert plan.bm_rows_total == 44 and plan.ops.shape[0] >= 2 and (plan.ops[:, 3] == 1).all()
    got = bc.restate_place_templates(arrays[("Car", 7, 0)], plan.bm_first, plan.bm_rows, plan.bm_place, plan.bm_offsets, plan.ops, plan.op_offsets)
    assert got.tobytes() == np.ascontiguousarray(want, np.float32).tobytes()


SIGNED_ZERO_ROWS = [[0.0, 0.0, -0.0], [-0.0, -0.0, -0.0], [0.0, -0.0, 1.0], [-0.0, 0.0, -1.0], [1.25, -0.5, -0.0]]


def _einsum_templates(rng, n):
    """n == 1: each signed-zero row as a template of its own (the first has z = -0.0 and x = y = 0); else one random template that holds them all"""
    if n == 1:
        return [np.array([r], np.float32) for r in SIGNED_ZERO_ROWS]
    t = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    t[:5] = SIGNED_ZERO_ROWS
    return [t[rng.permutation(n)]]


@pytest.mark.parametrize("n", [1, 44, 45, 1000])
def test_restatement_equals_einsum(n):
    """the header's arithmetic against np.einsum("nj,ij->ni", t, R) + centre itself, on random float32 templates that hold rows with
    z = -0.0 and x = y = 0 in either sign, for yaw 0, +-pi/2, pi and two oblique ones, and centres whose zeros have either sign (where the
    sign of a zero sum shows: einsum accumulates from +0)"""
    from btcdet_amd import data_side
    rng = np.random.default_rng(n)
    for yaw in (0.0, np.pi / 2, -np.pi / 2, np.pi, 0.3, -2.1):
        for centre in ([1.5, -2.0, 0.25], [0.0, -0.0, 0.0], [-0.0, -0.0, -0.0]):
            for t in _einsum_templates(rng, n):
                box = np.array(centre + [3.9, 1.6, 1.5, yaw], np.float32)
                R = data_side.get_yaw_rotation(box[6])
                assert R.dtype == np.float32
                want = np.einsum("nj,ij->ni", t, R) + box[:3]
                got = bc.restate_rows(t, (R[0, 0], R[0, 1], R[1, 0], box[0], box[1], box[2]))
                assert want.dtype == np.float32 and got.shape == (n, 3) and got.tobytes() == want.tobytes(), (n, yaw, centre)


def test_missing_template_raises(tmp_path, host_iou):
    from btcdet_amd.device_augmentor import DeviceAugmentor, TemplateBank
    aug, bank, arrays, roots = bc.build(tmp_path, "model")
    gone = dict(arrays)
    del gone[("Car", 7, 1)]
    dev = DeviceAugmentor(aug, bank, TemplateBank.from_arrays(gone))
    np.random.seed(ac.SEED)
    with pytest.raises(KeyError, match=re.escape(str(roots["Car"].resolve() / "7_1.pkl"))):
        dev.plan(_no_scan(bc.scenes()[:1]))


def test_float64_boxes_take_the_host_route(tmp_path, host_iou):
    from btcdet_amd.device_augmentor import DeviceAugmentor, TemplateBank
    scenes = bc.scenes()[:2]
    scenes[1]["gt_boxes"] = scenes[1]["gt_boxes"].astype(np.float64)
    aug0, bank0, _, _ = bc.build(tmp_path, "model")
    np.random.seed(ac.SEED)
    plain = DeviceAugmentor(aug0, bank0).plan(_no_scan(scenes))
    aug, bank, arrays, _ = bc.build(tmp_path, "model")
    np.random.seed(ac.SEED)
    plan = DeviceAugmentor(aug, bank, TemplateBank.from_arrays(arrays)).plan(_no_scan(scenes))
    assert plan.bm_device == [True, False] and plan.bm_offsets.tolist() == [0, plan.bm_first.shape[0], plan.bm_first.shape[0]]
    assert "bm_points" not in plan.special[0]
    assert plan.special[1]["bm_points"].shape[0] > 0 and plan.special[1]["bm_points"].tobytes() == plain.special[1]["bm_points"].tobytes()
    assert plan.bm_rows_total == plain.special[0]["bm_points"].shape[0]
    for a, b in zip(plan.scenes, plain.scenes):
        assert sorted(a) == sorted(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def test_ablation_stays_unimplemented(tmp_path):
    from btcdet_amd.device_augmentor import DataAugmentor
    cfg = bc.bm_cfg()
    cfg["ABLATION"] = ac.ED(RMV_MISS=True)
    with pytest.raises(NotImplementedError):
        DataAugmentor(tmp_path, [cfg], ac.CLASSES)


# ------------------------------------------------------------------------------------------------------------------- C ABI
def test_ctypes_table_matches_the_header():
    from btcdet_amd import _lib
    src = open(os.path.join(ROOT, "include", "btcdet_hip_bestmatch.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.BESTMATCH_EXPORTED_SYMBOLS) == ["btc_place_templates"]
    L = _lib.lib()
    kinds = {"int": _lib.ci, "long long": ctypes.c_longlong, "size_t": _lib.sz}
    for n in names:
        assert hasattr(L, n)
        res, args = _lib._BESTMATCH_SIGS[n]
        m = re.search(r"(size_t|int)\s+%s\s*\(([^)]*)\)" % n, src)
        assert kinds[m.group(1)] is res, n
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args) == 15, n
        for p, a in zip(params, args):
            want = _lib.vp if "*" in p else kinds[re.sub(r"\s+\w+$", "", p).replace("const ", "").strip()]
            assert a is want, (n, p)
    for other in ("btcdet_hip.h", "btcdet_hip_infer.h", "btcdet_hip_augment.h"):
        assert "btc_place_templates" not in open(os.path.join(ROOT, "include", other)).read()


P = 0x1000      # a non-null address nobody reads: every call below returns from its argument checks


def test_argument_checks_return_before_any_launch():
    from btcdet_amd import _lib
    L = _lib.lib()
    out = np.full((16, 4), np.float32(-7.5))

    def call(bank=P, bank_rows=50, first=P, rows=P, place=P, offs=P, row_offs=P, n_pl=3, batch=2, ops=P, op_offs=P, n_out=16, ld=3, o=out.ctypes.data):
        return L.btc_place_templates(bank, bank_rows, first, rows, place, offs, row_offs, n_pl, batch, ops, op_offs, n_out, ld, o, None)
    for ld in (2, 5, 0, -3):
        assert call(ld=ld) == -1 and b"out_ld 3" in L.btc_last_error(), ld
    for batch in (0, -1):
        assert call(batch=batch) == -1 and b"batch >= 1" in L.btc_last_error()
    for kw in (dict(n_pl=-1), dict(bank_rows=-1), dict(n_out=-1)):
        assert call(**kw) == -1 and b"negative count" in L.btc_last_error(), kw
    assert call(n_out=2 ** 31) == -1 and b"31 bits" in L.btc_last_error()
    for kw in ("offs", "row_offs", "op_offs"):
        assert call(**{kw: None}) == -1 and b"missing pointer (bm_offsets, bm_row_offsets or op_offsets)" in L.btc_last_error(), kw
    for kw in ("bank", "first", "rows", "place"):
        assert call(**{kw: None}) == -1 and b"missing pointer (bank or bm_*)" in L.btc_last_error(), kw
    assert call(o=None) == -1 and b"missing pointer (out)" in L.btc_last_error()
    assert (out == np.float32(-7.5)).all()
    # nothing to do, nothing launched: no placement needs no bank, no row needs no out, and ops may always be NULL
    assert call(n_out=0, o=None) == 0
    assert call(n_out=0, n_pl=0, bank=None, first=None, rows=None, place=None, ops=None, o=None) == 0
    assert (out == np.float32(-7.5)).all()
