"""btcdet_amd/kitti_infos.py without a GPU, against what the reference's own get_infos and create_info_file_with_coverage produced over
the synthetic directory (tests/golden/kitti_infos.npz): the label parser and every host-made info field, PNG headers, the numpy
restatement of include/btcdet_hip_infos.h (kitti_infos_ref.restate_counts / restate_cells) against the reference's counts and rates,
get_infos without labels or counts, the coverage_rates shapes, KittiFrames(infos=...) and the pickle round trip; the ctypes table
against the header."""
import os
import pickle
import re

import numpy as np
import pytest

import kitti_frames_ref as kr
import kitti_infos_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def raw_dir(tmp_path_factory):
    return ir.build_dir(ir.gold(), tmp_path_factory.mktemp("kitti_raw"))


@pytest.fixture(scope="module")
def plain_infos(raw_dir):
    from btcdet_amd.kitti_infos import KittiInfoBuilder
    return KittiInfoBuilder(raw_dir, "train").get_infos(has_label=True, count_inside_pts=False)


def _golden_infos():
    """the reference's infos rebuilt from the stored arrays, in its key order"""
    g = ir.gold()
    infos = []
    for k in range(ir.N_FRAMES):
        p = "info%d_" % k
        infos.append({"point_cloud": {"num_features": int(g[p + "num_features"]), "lidar_idx": str(g[p + "lidar_idx"])},
                      "image": {"image_idx": str(g[p + "image_idx"]), "image_shape": g[p + "image_shape"].copy()},
                      "calib": {key: g[p + "calib_" + key].copy() for key in ir.CALIB_KEYS},
                      "annos": {str(key): g[p + "anno_" + str(key)].copy() for key in g[p + "anno_keys"]}})
    return infos


def _blocks(k):
    c = kr.parse_calib(ir.gold()["f%d_calib_txt" % k].tobytes().decode())
    H, W = ir.image_hw(k)
    return kr.calib_block(kr.lidar_to_rect_matrix(c["R0"], c["Tr_velo2cam"]), c["P2"], W, H)


def _restated_objects(k, infos):
    """frame k's database objects by gt_database_ref.restate_cut: what GtDatabase.build cuts on the GPU"""
    pts = ir.gold()["f%d_points" % k]
    out, bounds, _ = ir.gr.restate_cut(pts, [0, pts.shape[0]], [infos[k]["annos"]["gt_boxes_lidar"]])
    return [out[bounds[j]:bounds[j + 1]] for j in range(len(bounds) - 1)]


# ----------------------------------------------------------------------------------------------------------------------- labels
def test_label_parser_gives_the_reference_fields(plain_infos):
    g = ir.gold()
    for k, info in enumerate(plain_infos):
        annos = info["annos"]
        want_keys = [str(x) for x in g["info%d_anno_keys" % k] if str(x) != "num_points_in_gt"]
        assert list(annos.keys()) == want_keys
        for key in want_keys:
            want = g["info%d_anno_%s" % (k, key)]
            assert annos[key].dtype == want.dtype and annos[key].shape == want.shape and np.array_equal(annos[key], want), (k, key)
    levels = np.concatenate([x["annos"]["difficulty"] for x in plain_infos])
    assert set(levels.tolist()) == {-1, 0, 1, 2}, "Easy, Moderate, Hard and UnKnown all occur"
    assert plain_infos[1]["annos"]["score"][0] == 0.87 and np.all(plain_infos[0]["annos"]["score"] == -1.0)        # the 16-field line


def test_object3d_types_and_levels():
    from btcdet_amd.kitti_infos import Object3d
    o = Object3d("Car 0.10 0 -1.58 587.01 173.33 614.12 220.12 1.65 1.67 3.64 -0.65 1.71 46.70 -1.59\n")
    assert o.box2d.dtype == np.float32 and o.loc.dtype == np.float32 and o.box2d.shape == (4,) and o.loc.shape == (3,)
    assert all(type(v) is float for v in (o.truncation, o.occlusion, o.alpha, o.h, o.w, o.l, o.ry, o.score)) and o.score == -1.0
    assert (o.h, o.w, o.l) == (1.65, 1.67, 3.64) and o.level == 0

    def level(top, bottom, trunc, occ):
        return Object3d("Car %.2f %d 0 0 %.2f 50 %.2f 1 1 1 0 0 10 0" % (trunc, occ, top, bottom)).level
    assert [level(*a) for a in ir.LEVELS] == [0, 1, 2, -1, -1, -1]
    assert level(100.0, 139.0, 0.15, 0) == 0 and level(100.0, 138.99, 0.15, 0) == 1          # height = bottom - top + 1 >= 40
    assert Object3d("Car 0 0 0 0 0 1 50 1 1 1 0 0 10 0 0.5").score == 0.5


def test_image_shape_reads_the_png_header(tmp_path):
    from btcdet_amd.kitti_infos import image_shape
    for name, (h, w, grey) in {"rgb.png": (375, 1242, False), "grey.png": (3, 70000, True)}.items():
        (tmp_path / name).write_bytes(ir.png_bytes(h, w, grey))
        got = image_shape(tmp_path / name)
        assert got.dtype == np.int32 and got.tolist() == [h, w]
    (tmp_path / "short.png").write_bytes(ir.png_bytes(4, 4)[:20])
    (tmp_path / "not.png").write_bytes(b"\xff\xd8\xff\xe0" + b"\0" * 64)
    (tmp_path / "empty.png").write_bytes(b"")
    for name in ("short.png", "not.png", "empty.png"):
        with pytest.raises(ValueError, match=name):
            image_shape(tmp_path / name)


# ------------------------------------------------------------------------------------------------------------------ restatement
def test_restated_counts_are_the_reference_counts():
    g = ir.gold()
    for k in range(ir.N_FRAMES):
        pts, boxes = g["f%d_points" % k], g["info%d_anno_gt_boxes_lidar" % k]
        counts, fov = ir.restate_counts(pts, [0, pts.shape[0]], [_blocks(k)], [boxes])
        want = g["info%d_anno_num_points_in_gt" % k]
        print("frame", k, "in view", int(fov[0]), "counts", counts.tolist())
        assert np.array_equal(counts, want[:boxes.shape[0]]) and np.all(want[boxes.shape[0]:] == -1) and want.dtype == np.int32
    assert float(g["count_nearest"]) > 10.0 * float(g["count_dev"].max()), "the generator's margin"


def test_host_hull_rows_are_the_restated_rows():
    from btcdet_amd.kitti_infos import hull_rows
    b = ir.gold()["info0_anno_gt_boxes_lidar"]
    assert hull_rows(b).tobytes() == ir.hull_rows(b).tobytes() and hull_rows(b).dtype == np.float32
    assert np.array_equal(hull_rows(b)[:, 3], (b[:, 3].astype(np.float32) / np.float32(2.0)))


def test_restated_cells_and_the_host_fallback_are_the_reference_rates():
    from btcdet_amd.kitti_infos import coverage_cells_host
    g = ir.gold()
    infos = _golden_infos()
    j = 0
    for k, info in enumerate(infos):
        objs = _restated_objects(k, infos)
        for i, name in enumerate(info["annos"]["name"]):
            rate = g["cov%d" % k].reshape(-1)[i]
            if name not in ir.COVERAGE_CLASSES:
                assert rate == 0.0
                continue
            box = info["annos"]["gt_boxes_lidar"][i]
            uo, ub, st = ir.restate_cells(g["tmpl_%d_%d" % (k, i)], objs[i], ir.pose_of(box))
            assert st == 0 and (uo, ub) == tuple(g["cells"][j]) and rate == uo / max(1, ub), (k, i)
            assert coverage_cells_host(g["tmpl_%d_%d" % (k, i)], objs[i], box) == (uo, ub)
            j += 1
    assert j == g["cells"].shape[0]
    assert float(g["cell_nearest"]) > max(10.0 * float(g["cell_dev"]), 1e-9), "the generator's margin"


def test_restated_cells_flag_a_wide_job():
    t = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.2]], np.float32)
    far = ir.pose_of(np.array([330.0, 0, 0, 4, 2, 2, 0.3]))
    assert ir.restate_cells(t, t, far) == (None, None, 1)
    assert ir.restate_cells(t, t, ir.pose_of(np.array([300.0, 0, 0, 4, 2, 2, 0.3])))[2] == 0
    assert ir.restate_cells(np.zeros((0, 3), np.float32), t, far) == (0, 0, 0)


# ------------------------------------------------------------------------------------------------------------------- the builder
def test_get_infos_without_counts_or_labels_needs_no_gpu(raw_dir, plain_infos):
    from btcdet_amd.kitti_infos import KittiInfoBuilder
    g = ir.gold()
    b = KittiInfoBuilder(raw_dir, "train")
    assert b.sample_id_list == ir.FRAME_IDS
    test_infos = b.get_infos(has_label=False)
    ir.assert_infos_equal(test_infos, g, "test", n_frames=ir.N_FRAMES)
    assert all(list(x.keys()) == ["point_cloud", "image", "calib"] for x in test_infos)
    for info in plain_infos:                          # the golden infos minus the counts
        info = dict(info, annos=dict(info["annos"]))
        k = ir.FRAME_IDS.index(info["point_cloud"]["lidar_idx"])
        info["annos"]["num_points_in_gt"] = g["info%d_anno_num_points_in_gt" % k]
        ir.assert_infos_equal([info], g, "info", frame_map=[k])
    some = b.get_infos(has_label=False, sample_id_list=["000042", "000003"])
    assert [x["point_cloud"]["lidar_idx"] for x in some] == ["000042", "000003"]
    assert g["info0_calib_P2"].dtype == np.float64 and g["info0_calib_R0_rect"].dtype == np.float32 and g["info0_calib_Tr_velo_to_cam"].dtype == np.float64
    assert g["info0_anno_gt_boxes_lidar"].dtype == np.float64 and g["info4_anno_gt_boxes_lidar"].shape == (0, 7)


def test_an_empty_label_file_is_named(raw_dir, tmp_path):
    from btcdet_amd.kitti_infos import KittiInfoBuilder
    root = ir.build_dir(ir.gold(), tmp_path)
    open(os.path.join(root, "training", "label_2", "000010.txt"), "w").close()
    with pytest.raises(ValueError, match="000010.txt"):
        KittiInfoBuilder(root, "train").get_infos(count_inside_pts=False)


# ---------------------------------------------------------------------------------------------------------------------- coverage
def test_coverage_rate_shapes():
    from btcdet_amd.kitti_infos import coverage_rate_array
    a0, a1, a3 = coverage_rate_array([]), coverage_rate_array([0.25]), coverage_rate_array([0.0, 0.5, 8.0])
    assert a0.shape == (0, 1) and a0.dtype == np.float32
    assert a1.shape == (1, 1) and a1.dtype == np.float64 and a1[0, 0] == 0.25
    assert a3.shape == (3,) and a3.dtype == np.float64 and a3.tolist() == [0.0, 0.5, 8.0]


def test_add_coverage_with_the_restatement_gives_the_reference_field():
    from btcdet_amd.device_augmentor import TemplateBank
    from btcdet_amd.gt_database import GtDatabase
    from btcdet_amd.kitti_infos import add_coverage
    g = ir.gold()
    infos = _golden_infos()
    db = GtDatabase.from_arrays(infos, [_restated_objects(k, infos) for k in range(ir.N_FRAMES)], split="train")
    templates = TemplateBank.from_arrays(ir.template_arrays(g))
    out = add_coverage(infos, db.bank, templates, "train", cells_fn=lambda jobs, pose: ir.restate_jobs(templates.rows, db.bank.rows, jobs, pose))
    for k, info in enumerate(out):
        got, want = info["annos"]["coverage_rates"], g["cov%d" % k]
        assert list(info["annos"].keys())[-1] == "coverage_rates"
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (k, got, want)
    # a flagged job goes through the host route: flag every job
    again = add_coverage(_golden_infos(), db.bank, templates, "train",
                         cells_fn=lambda jobs, pose: (np.zeros((len(jobs), 2), np.int32), np.ones((len(jobs),), np.int32)))
    assert all(np.array_equal(a["annos"]["coverage_rates"], g["cov%d" % k]) for k, a in enumerate(again))
    # a missing template, a missing database entry: a KeyError that names the object
    fewer = dict(ir.template_arrays(g))
    del fewer[("Cyclist", 7, 0)]
    with pytest.raises(KeyError, match="7_0.pkl"):
        add_coverage(_golden_infos(), db.bank, TemplateBank.from_arrays(fewer), "train", cells_fn=lambda j, p: None)
    with pytest.raises(KeyError, match="gt_database_val/000003_Car_0.bin"):
        add_coverage(_golden_infos(), db.bank, templates, "val", cells_fn=lambda j, p: None)


# ------------------------------------------------------------------------------------------------------------------ KittiFrames
def test_kitti_frames_takes_the_infos_in_memory(raw_dir, tmp_path):
    from btcdet_amd.kitti_frames import KittiFrames
    infos = _golden_infos()
    with pytest.raises(FileNotFoundError):
        KittiFrames(raw_dir, "train")                                          # no pickle in a raw directory
    mem = KittiFrames(raw_dir, "train", infos=infos)
    assert mem.infos is infos and len(mem) == ir.N_FRAMES and mem.sample_id_list == ir.FRAME_IDS
    root = ir.build_dir(ir.gold(), tmp_path)
    with open(os.path.join(root, "kitti_infos_train.pkl"), "wb") as f:           # what create_kitti_infos writes: pickle.dump of the list
        pickle.dump(infos, f)
    disk = KittiFrames(root, "train")
    for i in range(len(mem)):
        a, b = mem.scene(i), disk.scene(i)
        assert a.keys() == b.keys() and a["frame_id"] == b["frame_id"]
        assert np.array_equal(a["gt_boxes"], b["gt_boxes"]) and np.array_equal(a["gt_names"], b["gt_names"]) and np.array_equal(a["image_shape"], b["image_shape"])
        assert np.array_equal(mem.fov_crop_host(i), disk.fov_crop_host(i))
    assert np.array_equal(mem.calib_blocks(range(len(mem))), disk.calib_blocks(range(len(disk))))
    assert np.array_equal(mem.calib_blocks([2])[0], _blocks(2))
    ir.assert_infos_equal(disk.infos, ir.gold(), "info", n_frames=ir.N_FRAMES)   # the round trip keeps every dtype


# ------------------------------------------------------------------------------------------------------------------------- C ABI
def test_ctypes_table_matches_the_header():
    from btcdet_amd import _lib
    src = open(os.path.join(ROOT, "include", "btcdet_hip_infos.h")).read()
    for line in ("x = (tx*c - ty*s) + cx,  y = (tx*s + ty*c) + cy,  z = tz + cz", "r  = sqrt((x*x + y*y) + z*z)", "az = (atan2(-y, x) * 180.0) / pi",
                 "el = (atan2(z, sqrt(x*x + y*y)) * 180.0) / pi", "cell_k = floor((s_k - mn_k) / res_k),  res = (0.32, 0.5184, 0.4203125)",
                 "(|z - cz| <= hz) & (|lx| < hx) & (|ly| < hy)"):
        assert line in src, "the header states its formulas: " + line
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.INFOS_EXPORTED_SYMBOLS) == ["btc_count_in_boxes", "btc_count_in_boxes_ws_bytes", "btc_coverage_cells",
                                                           "btc_coverage_cells_ws_bytes"]
    L = _lib.lib()
    kinds = {"int": _lib.ci, "size_t": _lib.sz}
    for n, count in (("btc_count_in_boxes", 14), ("btc_count_in_boxes_ws_bytes", 2), ("btc_coverage_cells", 14), ("btc_coverage_cells_ws_bytes", 2)):
        assert hasattr(L, n)
        res, args = _lib._INFOS_SIGS[n]
        m = re.search(r"(size_t|int)\s+%s\s*\(([^)]*)\)" % n, src)
        assert kinds[m.group(1)] is res, n
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args) == count, n
        for p, a in zip(params, args):
            want = _lib.vp if "*" in p else kinds[re.sub(r"\s+\w+$", "", p).replace("const ", "").strip()]
            assert a is want, (n, p)
    for other in ("btcdet_hip.h", "btcdet_hip_infer.h", "btcdet_hip_augment.h", "btcdet_hip_bestmatch.h", "btcdet_hip_frames.h", "btcdet_hip_gtdb.h",
                  "btcdet_hip_templates.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
        assert not set(names) & set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", text)), other
    assert L.btc_count_in_boxes_ws_bytes(-1, 1) == 0 and L.btc_count_in_boxes_ws_bytes(10, 0) == 0 and L.btc_count_in_boxes_ws_bytes(10, 3) > 0
    assert L.btc_coverage_cells_ws_bytes(-1, 10) == 0 and L.btc_coverage_cells_ws_bytes(3, -1) == 0 and L.btc_coverage_cells_ws_bytes(3, 2 ** 29) == 0
    assert L.btc_coverage_cells_ws_bytes(7, 4096) == 256 and L.btc_coverage_cells_ws_bytes(7, 4097) == 7 * 16384 * 4
    assert _lib.ci is not None and ir.SPHERE_RES.tolist() == [0.32, 0.5184, 0.4203125]
