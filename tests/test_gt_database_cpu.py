"""btcdet_amd/gt_database.py without a GPU: the numpy restatement of include/btcdet_hip_gtdb.h (gt_database_ref.restate_cut) plus the host
bookkeeping reproduce what the reference's own create_groundtruth_database wrote (tests/golden/gt_database.npz: every file's bytes, every
db_info field, with and without used_classes); save() round-trips through the file-reading ObjectBank and through pickle;
ObjectBank.from_rows; the layout of one cut (box_offsets, max_boxes, the second call's capacity, the 2^31 refusal); the KeyError of
infos without lidar boxes; the ctypes table against the header and the argument checks that return before any launch."""
import os
import pickle
import re

import numpy as np
import pytest

import gt_database_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _infos():
    return gr.infos_of(gr.gold())


def _objects(infos):
    """per info: the list of its objects' rows by the restatement"""
    g = gr.gold()
    per_frame = []
    for k, info in enumerate(infos):
        if "annos" not in info:
            per_frame.append([])
            continue
        pts = g["f%d_points" % k]
        out, bounds, _ = gr.restate_cut(pts, [0, pts.shape[0]], [info["annos"]["gt_boxes_lidar"]])
        per_frame.append([out[bounds[j]:bounds[j + 1]] for j in range(len(bounds) - 1)])
    return per_frame


@pytest.fixture(scope="module")
def host_db():
    from btcdet_amd.gt_database import GtDatabase
    infos = _infos()
    objs = _objects(infos)
    return {u: GtDatabase.from_arrays(infos, objs, used_classes=c) for u, c in (("all_", None), ("car_", ["Car"]))}


def _golden_files():
    g = gr.gold()
    ends = np.cumsum(g["file_sizes"])
    return [(str(n), g["file_bytes"][e - s:e].tobytes()) for n, s, e in zip(g["file_names"], g["file_sizes"], ends)]


def test_the_fixture_is_the_helper_directory():
    """the seeded directory of gt_database_ref is the one the reference ran over"""
    g, now = gr.gold(), gr.frames()
    assert all(np.array_equal(g[k], v) for k, v in now.items())
    assert float(g["dev"].max()) * 10 < gr.FACE_MARGIN
    for k in range(gr.N_FRAMES):
        if gr.HAS_ANNOS[k]:
            assert gr.face_distance(g["f%d_points" % k], g["f%d_anno_gt_boxes_lidar" % k]).min() > 10 * g["dev"][k]


def test_restatement_is_the_samplers_predicate():
    from btcdet_amd.database_sampler import points_in_boxes_mask
    from btcdet_amd.device_augmentor import removal_rows
    g = gr.gold()
    for k in range(gr.N_FRAMES):
        if not gr.HAS_ANNOS[k]:
            continue
        pts, boxes = g["f%d_points" % k], g["f%d_anno_gt_boxes_lidar" % k]
        rows = gr.box_rows(boxes)
        assert rows.tobytes() == removal_rows(boxes.astype(np.float32)).tobytes()
        mask = np.stack([gr.restate_mask(pts, r) for r in rows])
        assert np.array_equal(mask, points_in_boxes_mask(pts[:, 0:3], boxes.astype(np.float32)))
        print("frame", k, "rows per box", mask.sum(axis=1).tolist())
    m0 = np.stack([gr.restate_mask(g["f0_points"], r) for r in gr.box_rows(g["f0_anno_gt_boxes_lidar"])])
    assert m0[3].sum() == 0 and m0[4].sum() == 1 and (m0[0] & m0[1]).sum() > 0


def test_exact_case_on_the_faces():
    from btcdet_amd.database_sampler import points_in_boxes_mask
    box, pts, expect = gr.exact_case()
    assert np.array_equal(gr.gold()["exact_inside"], expect)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(gr.restate_mask(pts, gr.box_rows(box)[0]), expect)
        assert np.array_equal(points_in_boxes_mask(pts[:, 0:3], box)[0], expect)
    out, bounds, src = gr.restate_cut(pts, [0, len(pts)], [box])
    assert src.tolist() == np.flatnonzero(expect).tolist() and bounds.tolist() == [0, int(expect.sum())]


@pytest.mark.parametrize("prefix", ["all_", "car_"])
def test_host_bookkeeping_reproduces_the_reference(host_db, prefix):
    db = host_db[prefix]
    gr.assert_db_infos_equal(db.db_infos, gr.gold(), prefix)
    files = _golden_files()
    assert [p for p, _, _ in db.objects] == ["gt_database/" + n for n, _ in files]
    rows = db.bank.rows
    for (path, first, n), (_, data) in zip(db.objects, files):
        assert rows[first:first + n].tobytes() == data, path
        assert db.bank.table[path] == (first, n)
    assert db.num_points.tolist() == [len(d) // 16 for _, d in files]
    car = db.db_infos["Car"][0]
    assert type(car["path"]) is str and type(car["gt_idx"]) is int and type(car["num_points_in_gt"]) is int
    assert car["box3d_lidar"].dtype == np.float64 and isinstance(car["name"], np.str_) and isinstance(car["difficulty"], np.int32)
    if prefix == "all_":      # the literal names[i]: frame 000042's second box is filed under the name next to it in the annos
        assert [e["path"] for e in db.db_infos["DontCare"]] == ["gt_database/000042_DontCare_1.bin"]
        assert "gt_database/000042_Pedestrian_2.bin" in db.bank.table


def test_save_round_trips_through_the_file_reading_bank_and_pickle(host_db, tmp_path):
    from btcdet_amd.device_augmentor import ObjectBank
    db = host_db["all_"]
    pkl = db.save(tmp_path)
    assert pkl == tmp_path / "kitti_dbinfos_train.pkl"
    for name, data in _golden_files():
        assert (tmp_path / "gt_database" / name).read_bytes() == data, name
    assert sorted(os.listdir(tmp_path / "gt_database")) == sorted(n for n, _ in _golden_files())
    with open(pkl, "rb") as f:
        back = pickle.load(f)
    gr.assert_db_infos_equal(back, gr.gold(), "all_")
    bank = ObjectBank(tmp_path, back, 4)
    for entries in back.values():
        for e in entries:
            f0, n0 = bank.table[e["path"]]
            f1, n1 = db.bank.table[e["path"]]
            assert n0 == n1 == e["num_points_in_gt"] and bank.rows[f0:f0 + n0].tobytes() == db.bank.rows[f1:f1 + n1].tobytes()
    with pytest.raises(ValueError, match="built for split"):
        db.save(tmp_path, split="val")


def test_object_bank_from_rows():
    from btcdet_amd.device_augmentor import ObjectBank
    rows = np.arange(40, dtype=np.float32).reshape(10, 4)
    bank = ObjectBank.from_rows(rows, {"a": (0, 3), "b": (3, 7)}, 4)
    assert bank.rows.tobytes() == rows.tobytes() and bank.table == {"a": (0, 3), "b": (3, 7)} and bank.num_point_features == 4
    assert bank.tensor("cpu").numpy().tobytes() == rows.tobytes() and bank.tensor("cpu") is bank.tensor("cpu")
    with pytest.raises(AssertionError):
        ObjectBank.from_rows(rows, {"a": (8, 3)}, 4)
    with pytest.raises(ValueError):
        ObjectBank.from_rows(None, {}, 4)
    import torch
    t = torch.from_numpy(rows.copy())
    lazy = ObjectBank.from_rows(None, {"a": (0, 10)}, 4, device_rows=t)
    assert lazy._rows is None and lazy.tensor("cpu") is t            # the resident tensor itself, no copy
    assert lazy.rows.tobytes() == rows.tobytes() and lazy._rows is not None


def test_cut_layout_and_the_second_call():
    from btcdet_amd.device_augmentor import removal_rows
    from btcdet_amd.gt_database import cut_layout, second_capacity
    rng = np.random.default_rng(5)
    boxes = [rng.uniform(1, 5, (3, 7)), np.zeros((0, 7)), rng.uniform(1, 5, (5, 7)), rng.uniform(1, 5, (1, 7))]
    lay = cut_layout([0, 10, 10, 300, 301], boxes)
    assert lay["box_offsets"].tolist() == [0, 3, 3, 8, 9] and lay["box_offsets"].dtype == np.int32
    assert lay["max_boxes"] == 5 and lay["m"] == 9 and lay["n"] == 301 and lay["scene_offsets"].dtype == np.int32
    allb = np.concatenate(boxes)
    assert lay["rows"].tobytes() == removal_rows(allb.astype(np.float32)).tobytes() and lay["rows"].shape == (9, 8)
    assert lay["centre"].dtype == np.float64 and lay["centre"].tobytes() == np.ascontiguousarray(allb[:, :3]).tobytes()      # as given, not via float32
    other = [np.ones((b.shape[0], 3), np.float32) for b in boxes]
    assert cut_layout([0, 10, 10, 300, 301], boxes, other)["centre"].tolist() == np.ones((9, 3)).tolist()
    empty = cut_layout([0, 7], [np.zeros((0, 7))])
    assert empty["max_boxes"] == 0 and empty["m"] == 0 and empty["rows"].shape == (0, 8) and empty["box_offsets"].tolist() == [0, 0]
    assert second_capacity(10, 10) is None and second_capacity(0, 0) is None and second_capacity(11, 10) == 11
    for bad in ([0, 5], [1, 5, 9], [0, 9, 5]):
        with pytest.raises(ValueError):
            cut_layout(bad, boxes[:2])
    with pytest.raises(ValueError, match="one centre per box"):
        cut_layout([0, 5], [boxes[0]], [np.zeros((2, 3))])


def test_a_batch_of_two_to_the_31_pairs_is_refused_on_the_host():
    from btcdet_amd.gt_database import cut_layout
    boxes = np.ones((1 << 11, 7))
    rows = 1 << 19
    ok = cut_layout([0, rows, 2 * rows - 1], [boxes, boxes])             # 2^31 - 2^11 pairs
    assert ok["m"] == 1 << 12
    with pytest.raises(ValueError, match=r"reach 2\^31"):
        cut_layout([0, rows, 2 * rows], [boxes, boxes])                   # exactly 2^31


def test_infos_without_lidar_boxes_raise_a_keyerror_that_names_the_frame():
    from btcdet_amd.gt_database import GtDatabase
    infos = _infos()
    del infos[3]["annos"]["gt_boxes_lidar"]
    with pytest.raises(KeyError, match="000042"):
        GtDatabase.from_arrays(infos, [[]] * len(infos))
    assert GtDatabase.frame_boxes(infos[2]) is None                       # no annos: skipped, not an error


# ------------------------------------------------------------------------------------------------------------------------- C ABI
def test_ctypes_table_matches_the_header():
    from btcdet_amd import _lib
    src = open(os.path.join(ROOT, "include", "btcdet_hip_gtdb.h")).read()
    for line in ("sx = x - cx,  sy = y - cy", "lx = sx*c - sy*s,  ly = sx*s + sy*c", "inside = (|z - cz| <= hz) & (|lx| < hx) & (|ly| < hy)",
                 "(float)((double)p - centre[j])"):
        assert line in src, "the header states its formulas: " + line
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.GTDB_EXPORTED_SYMBOLS) == ["btc_cut_objects", "btc_cut_objects_ws_bytes"]
    L = _lib.lib()
    kinds = {"int": _lib.ci, "size_t": _lib.sz}
    for n, count in (("btc_cut_objects", 17), ("btc_cut_objects_ws_bytes", 4)):
        assert hasattr(L, n)
        res, args = _lib._GTDB_SIGS[n]
        m = re.search(r"(size_t|int)\s+%s\s*\(([^)]*)\)" % n, src)
        assert kinds[m.group(1)] is res, n
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args) == count, n
        for p, a in zip(params, args):
            want = _lib.vp if "*" in p else kinds[re.sub(r"\s+\w+$", "", p).replace("const ", "").strip()]
            assert a is want, (n, p)
    for other in ("btcdet_hip.h", "btcdet_hip_infer.h", "btcdet_hip_augment.h", "btcdet_hip_bestmatch.h", "btcdet_hip_frames.h"):
        assert "btc_cut_objects" not in open(os.path.join(ROOT, "include", other)).read()


P = 0x1000      # a non-null address nobody reads: every call below returns from its argument checks


def test_argument_checks_return_before_any_launch():
    from btcdet_amd import _lib
    L = _lib.lib()
    ws = L.btc_cut_objects_ws_bytes
    assert ws(-1, 1, 1, 1) == 0 and ws(5, 0, 1, 1) == 0 and ws(5, 1, -1, 1) == 0 and ws(5, 1, 1, -1) == 0
    small, big = ws(0, 1, 0, 0), ws(120000, 2, 30, 20)
    assert 0 < small < big and big >= (120000 // 256 + 2) * 20 * 4 and ws(120000, 2, 30, 40) > big
    assert ws(2 ** 31 - 1, 64, 4096, 255) > 2 ** 31                    # sized in size_t

    def call(pts=P, n=300, ld=4, offs=P, batch=2, boxes=P, centre=P, box_offs=P, m=3, max_boxes=2, cap=300, out=P, obj_offs=P, src=None, ws_ptr=P,
             ws_bytes=1 << 20):
        return L.btc_cut_objects(pts, n, ld, offs, batch, boxes, centre, box_offs, m, max_boxes, cap, out, obj_offs, src, ws_ptr, ws_bytes, None)
    for ld in (2, 0, -3):
        assert call(ld=ld) == -1 and b"ld >= 3" in L.btc_last_error(), ld
    for batch in (0, -1):
        assert call(batch=batch) == -1 and b"batch >= 1" in L.btc_last_error()
    for kw in (dict(n=-1), dict(m=-1), dict(max_boxes=-1), dict(cap=-1)):
        assert call(**kw) == -1 and b"negative count" in L.btc_last_error(), kw
    for kw in ("offs", "box_offs", "obj_offs", "ws_ptr"):
        assert call(**{kw: None}) == -1 and b"missing pointer (scene_offsets, box_offsets, obj_offsets or ws)" in L.btc_last_error(), kw
    assert call(pts=None) == -1 and b"missing pointer (points)" in L.btc_last_error()
    for kw in ("boxes", "centre"):
        assert call(**{kw: None}) == -1 and b"missing pointer (boxes or centre)" in L.btc_last_error(), kw
    assert call(out=None) == -1 and b"missing pointer (out)" in L.btc_last_error()
    need = ws(300, 2, 3, 2)
    for ws_bytes in (0, 8, need - 1):
        assert call(ws_bytes=ws_bytes) == -1 and b"workspace too small" in L.btc_last_error(), ws_bytes
