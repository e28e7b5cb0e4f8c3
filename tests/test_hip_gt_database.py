"""btc_cut_objects (csrc/gt_database.hip, include/btcdet_hip_gtdb.h) through the C ABI against the numpy restatement of the header
(gt_database_ref.restate_cut: one float32 operation per rounded step), and GtDatabase.build against what the reference's own
create_groundtruth_database wrote (tests/golden/gt_database.npz).  Everything is exact: rows, order, bytes, obj_offsets, src_idx.

The shapes are the smallest at which the kernel can go wrong: scenes of 0 / 1 / 255 / 256 / 257 rows (one tile is 256 rows, tiles are
aligned to scenes), several scenes inside one 256-row span, a scene without boxes between two with boxes, 0 / 1 / 64 / 65 boxes in a
scene (64 are staged per pass), ld 3 / 4 / 5 and a base pointer off 16 bytes (the scalar path), an empty object, an object that takes
every row, a row in two objects, out_capacity below the total, max_boxes at and below the maximum, and the exact case on the faces.
The one-wave scans take 64 values at a time: 63 / 129 objects in all, a scene of 65 tiles, 65 scenes."""
import copy
import pickle

import numpy as np
import pytest
import torch

import gt_database_ref as gr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = np.float32(-7.5)


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def make_boxes(rng, n):
    """n boxes inside a 30 m x 20 m patch (they may overlap: a row may be in several objects)"""
    return np.stack([rng.uniform(5, 35, n), rng.uniform(-10, 10, n), rng.uniform(-1.2, -0.4, n), rng.uniform(3.2, 4.6, n), rng.uniform(1.5, 1.9, n),
                     rng.uniform(1.4, 1.9, n), rng.uniform(-3.1, 3.1, n)], axis=1).reshape(n, 7)


def make_scene(seed, n, nbox, ld=4):
    """-> (points (n, ld) f32, boxes (nbox, 7) f64): a third of the rows over the patch, the rest around the boxes out to 1.2 x their
    extents (a little over half of those inside), shuffled"""
    rng = np.random.default_rng(seed)
    boxes = make_boxes(rng, nbox)
    p = np.empty((n, 4), np.float32)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = rng.uniform(0, 40, n), rng.uniform(-15, 15, n), rng.uniform(-3.0, 1.5, n), rng.uniform(0, 1, n)
    if nbox:
        near = np.flatnonzero(rng.uniform(0, 1, n) < 0.67)
        b = boxes[rng.integers(0, nbox, near.size)]
        loc = rng.uniform(-1.2, 1.2, (near.size, 3)) * (b[:, 3:6] / 2)
        c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
        p[near, 0], p[near, 1], p[near, 2] = b[:, 0] + loc[:, 0] * c - loc[:, 1] * s, b[:, 1] + loc[:, 0] * s + loc[:, 1] * c, b[:, 2] + loc[:, 2]
    if ld == 3:
        p = np.ascontiguousarray(p[:, :3])
    elif ld > 4:
        p = np.concatenate([p, rng.uniform(0, 1, (n, ld - 4)).astype(np.float32)], axis=1)
    return p, boxes


def make_batch(sizes, nboxes, ld=4, seed=0):
    parts = [make_scene(1000 * seed + 10 * b + ld, s, nb, ld) for b, (s, nb) in enumerate(zip(sizes, nboxes))]
    return np.concatenate([p for p, _ in parts]).reshape(-1, ld), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), [b for _, b in parts]


def run(pts, offsets, boxes, cap=None, misalign=False, want_src=True, max_boxes=None, centres=None):
    """one btc_cut_objects call -> (out untrimmed (cap, ld), obj_offsets (m+1), src_idx untrimmed or None) as numpy; out and src_idx
    are poisoned first, so a slot the kernel left alone shows"""
    from btcdet_amd._lib import check, stream_ptr
    from btcdet_amd.gt_database import cut_layout
    lay = cut_layout(offsets, boxes, centres)
    n, ld = pts.shape
    B, m = len(boxes), lay["m"]
    max_boxes = lay["max_boxes"] if max_boxes is None else max_boxes
    cap = n if cap is None else cap
    shift = 1 if misalign else 0                                   # 4 bytes off a 16-byte boundary
    flat = torch.zeros((n * ld + 8,), dtype=torch.float32, device=DEV)
    flat[shift:shift + n * ld] = torch.from_numpy(pts.reshape(-1)).to(DEV)
    src_pts = flat[shift:shift + n * ld]
    oflat = torch.full((cap * ld + 8,), float(POISON), dtype=torch.float32, device=DEV)
    out = oflat[shift:shift + cap * ld]
    assert n == 0 or (src_pts.data_ptr() % 16 != 0) == misalign
    t = {k: torch.from_numpy(np.ascontiguousarray(lay[k])).to(DEV) for k in ("rows", "centre", "box_offsets", "scene_offsets")}
    obj_offs = torch.full((m + 1,), -9, dtype=torch.int32, device=DEV)
    idx = torch.full((max(cap, 1),), -9, dtype=torch.int32, device=DEV) if want_src else None
    ws_bytes = L().btc_cut_objects_ws_bytes(n, B, m, max_boxes)
    ws = torch.full((max(ws_bytes, 256),), 0xA5, dtype=torch.uint8, device=DEV)
    check(L().btc_cut_objects(src_pts.data_ptr() if n else None, n, ld, t["scene_offsets"].data_ptr(), B, t["rows"].data_ptr() if m else None,
                              t["centre"].data_ptr() if m else None, t["box_offsets"].data_ptr(), m, max_boxes, cap, out.data_ptr() if cap else None,
                              obj_offs.data_ptr(), idx.data_ptr() if want_src else None, ws.data_ptr(), ws_bytes, stream_ptr()), "btc_cut_objects")
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(cap, ld), obj_offs.cpu().numpy(), (idx.cpu().numpy()[:cap] if want_src else None)


def check_case(pts, offsets, boxes, cap=None, **kw):
    want, want_offs, want_src = gr.restate_cut(pts, offsets, boxes, kw.get("centres"))
    total = int(want_offs[-1])
    cap = max(total, 1) if cap is None else cap                     # by default everything fits (a row in two objects: total may exceed n)
    full, bounds, src = run(pts, offsets, boxes, cap=cap, **kw)
    print("rows", np.diff(offsets).tolist(), "boxes", [len(b) for b in boxes], "ld", pts.shape[1], "cap", cap, "per object", np.diff(want_offs).tolist(),
          {k: v for k, v in kw.items() if k != "centres"})
    assert bounds.tolist() == want_offs.tolist(), "obj_offsets are the true offsets whatever the capacity"
    held = min(total, cap)
    assert full[:held].tobytes() == want[:held].tobytes()
    assert (full[held:] == POISON).all(), "out written at or past min(total, out_capacity)"
    if src is not None:
        assert src[:held].tolist() == want_src[:held].tolist() and (src[held:] == -9).all()
    return want_offs


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_one_scene_around_a_tile(n):
    check_case(*make_batch([n], [3], seed=n % 5))


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "off16"])
@pytest.mark.parametrize("ld", [3, 4, 5])
def test_row_lengths_and_an_unaligned_base(ld, misalign):
    pts, offs, boxes = make_batch((257, 70, 300), (3, 2, 4), ld=ld, seed=1)
    want_offs = check_case(pts, offs, boxes, misalign=misalign)
    assert int(want_offs[-1]) > 100
    check_case(pts, offs, boxes, misalign=misalign, want_src=False)


@pytest.mark.parametrize("nbox", [0, 1, 60, 64, 65, 126])
def test_boxes_in_a_scene_around_a_staging_pass(nbox):
    """the scene of 600 rows (three tiles) owns nbox boxes; a scene in front of it and one behind own 2 and 1.  nbox = 60 and 126 make
    m = 63 and 129 objects: obj_offsets is a scan by one wave, 64 objects at a time, and 129 carries its running sum over two edges"""
    pts, offs, boxes = make_batch((100, 600, 50), (2, nbox, 1), seed=2)
    want_offs = check_case(pts, offs, boxes)
    if nbox:
        assert int(want_offs[2 + nbox] - want_offs[2]) > 100, "the boxes of the middle scene hold rows"


def test_a_scene_of_65_tiles():
    """a box's rows are counted per tile and scanned over its scene's tiles by one wave, 64 tiles at a time: 64 * 256 + 1 rows are 65
    tiles, the last of which starts from the sum of the first 64"""
    pts, offs, boxes = make_batch((64 * 256 + 1,), (2,), seed=9)
    pts[-1, :3] = boxes[0][0, :3]                                   # the one row of tile 64 sits at the first box's centre
    want_offs = check_case(pts, offs, boxes)
    assert (np.diff(want_offs) > 256).all(), "each box holds rows of several tiles"


def test_more_scenes_than_one_chunk_of_the_tile_scan():
    """tile_first is an exclusive scan over the scenes by one wave, 64 at a time: 65 scenes of 3 rows, every fourth with a box"""
    pts, offs, boxes = make_batch([3] * 65, [1 if b % 4 == 0 else 0 for b in range(65)], seed=10)
    pts[-1, :3] = boxes[64][0, :3]                                  # the last scene's box (behind the chunk edge) holds a row
    want_offs = check_case(pts, offs, boxes)
    assert int(np.diff(want_offs)[-1]) > 0 and (np.diff(want_offs) > 0).sum() > 4


def test_several_scenes_inside_one_span_and_a_scene_without_boxes_between():
    sizes = [20] * 9 + [0, 3, 60, 300]                              # 12 scenes inside the first 256 rows, one of them empty
    nboxes = [1, 2, 0, 3, 0, 0, 1, 2, 1, 2, 1, 0, 3]                # no boxes between scenes with boxes; boxes on an empty scene
    want_offs = check_case(*make_batch(sizes, nboxes, seed=3))
    assert (np.diff(want_offs) > 0).sum() > 8
    check_case(*make_batch([0, 0], [0, 0]))
    check_case(*make_batch([0, 5], [2, 0]))


def test_an_empty_object_one_that_takes_every_row_and_a_row_in_two_objects():
    pts, offs, boxes = make_batch((300, 257), (2, 1), seed=4)
    everything = np.array([[20.0, 0.0, 0.0, 200.0, 200.0, 40.0, 0.3]])
    nothing = np.array([[20.0, 0.0, 50.0, 4.0, 1.8, 1.6, 0.1]])
    boxes = [np.concatenate([boxes[0][:1], nothing, boxes[0][:1], everything, boxes[0][1:]]), np.concatenate([everything, boxes[1], everything])]
    want_offs = check_case(pts, offs, boxes)
    per = np.diff(want_offs).tolist()
    assert per[1] == 0 and per[3] == 300 and per[5] == per[7] == 257 and per[0] == per[2] > 0
    assert int(want_offs[-1]) > pts.shape[0], "more rows out than in: the total exceeds n"


def test_out_capacity_below_the_total():
    pts, offs, boxes = make_batch((300, 257, 40), (3, 2, 1), seed=5)
    total = int(gr.restate_cut(pts, offs, boxes)[1][-1])
    assert total > 200
    for cap in (total - 1, total // 2, 1, 0, total + 7):
        check_case(pts, offs, boxes, cap=cap)
        check_case(pts, offs, boxes, cap=cap, misalign=True)


def test_max_boxes_at_and_below_the_maximum():
    """max_boxes is exactly the largest scene's count on the product path; below it, the boxes of a scene past its first max_boxes get
    zero rows and the others are unchanged"""
    pts, offs, boxes = make_batch((300, 257), (4, 2), seed=6)
    want, want_offs, _ = gr.restate_cut(pts, offs, boxes)
    full, bounds, _ = run(pts, offs, boxes, cap=int(want_offs[-1]), max_boxes=4)
    assert bounds.tolist() == want_offs.tolist() and full.tobytes() == want.tobytes()
    per = np.diff(want_offs)
    for mb in (2, 0):
        keep = np.array([k < mb for b in boxes for k in range(len(b))])
        full, bounds, _ = run(pts, offs, boxes, cap=int(want_offs[-1]), max_boxes=mb)
        assert np.diff(bounds).tolist() == np.where(keep, per, 0).tolist()
        pieces = [want[want_offs[j]:want_offs[j + 1]] for j in np.flatnonzero(keep)]
        held = int(bounds[-1])
        assert full[:held].tobytes() == (np.concatenate(pieces).tobytes() if pieces else b"") and (full[held:] == POISON).all()


def test_centres_of_either_width_and_bits_that_are_no_numbers():
    """a float32 centre gives what numpy's float32 subtraction gives; columns 3.. are copied bit for bit on both paths"""
    pts, offs, boxes = make_batch((300,), (3,), seed=7)
    pts.view(np.uint32)[::3, 3] = 0x7FC12345
    pts.view(np.uint32)[1::3, 3] = 0x80000000
    c32 = [b[:, :3].astype(np.float32) for b in boxes]
    for misalign in (False, True):
        check_case(pts, offs, boxes, misalign=misalign)
        check_case(pts, offs, boxes, misalign=misalign, centres=c32)
    out, bounds, src = gr.restate_cut(pts, offs, boxes, c32)
    j = int(np.argmax(np.diff(bounds)))
    rows = pts[src[bounds[j]:bounds[j + 1]]].copy()
    rows[:, :3] -= c32[0][j]                                           # the reference's statement, float32 minus float32
    assert rows.tobytes() == out[bounds[j]:bounds[j + 1]].tobytes()


def test_exact_case_on_the_faces():
    box, pts, expect = gr.exact_case()
    assert np.array_equal(gr.gold()["exact_inside"], expect)
    for misalign in (False, True):
        full, bounds, src = run(pts, [0, len(pts)], [box], misalign=misalign)
        assert bounds.tolist() == [0, int(expect.sum())] and src[:bounds[1]].tolist() == np.flatnonzero(expect).tolist()
    # the same rows as the second of two scenes, behind a seeded one
    a, offs, boxes = make_batch((100,), (2,))
    check_case(np.concatenate([a, pts]), [0, 100, 100 + len(pts)], [boxes[0], box])


# ------------------------------------------------------------------------------------------------------------- GtDatabase.build
@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from btcdet_amd.gt_database import GtDatabase
    from btcdet_amd.kitti_frames import KittiFrames
    root = tmp_path_factory.mktemp("gtdb")
    gr.build_dir(gr.gold(), root)
    frames = KittiFrames(root, "train")
    return root, frames, {"all_": GtDatabase.build(frames, frames_per_batch=16, device=DEV),
                          "car_": GtDatabase.build(frames, used_classes=["Car"], frames_per_batch=2, device=DEV)}


def _golden_files():
    g = gr.gold()
    ends = np.cumsum(g["file_sizes"])
    return [(str(n), g["file_bytes"][e - s:e].tobytes()) for n, s, e in zip(g["file_names"], g["file_sizes"], ends)]


@pytest.mark.parametrize("prefix", ["all_", "car_"])
def test_build_gives_the_reference_files_and_db_infos(built, prefix):
    root, frames, dbs = built
    db = dbs[prefix]
    gr.assert_db_infos_equal(db.db_infos, gr.gold(), prefix)
    assert db.bank._rows is None and db.bank.tensor(DEV).is_cuda, "the rows have not left the device"
    rows = db.bank.tensor(DEV).cpu().numpy()
    files = _golden_files()
    assert [p for p, _, _ in db.objects] == ["gt_database/" + n for n, _ in files]
    for (path, first, n), (_, data) in zip(db.objects, files):
        assert rows[first:first + n].tobytes() == data, path
    assert db.num_points.tolist() == [len(d) // 16 for _, d in files]


def test_one_frame_per_batch_equals_all_frames_at_once(built):
    from btcdet_amd.gt_database import GtDatabase
    root, frames, dbs = built
    one = GtDatabase.build(frames, frames_per_batch=1, device=DEV)
    assert one.objects == dbs["all_"].objects
    assert torch.equal(one.bank.tensor(DEV).view(torch.int32), dbs["all_"].bank.tensor(DEV).view(torch.int32))
    assert pickle.dumps(one.db_infos) == pickle.dumps(dbs["all_"].db_infos)


def test_saved_database_reads_back_and_serves_the_augmentor(built):
    """save(): the file-reading ObjectBank holds per path the rows of the resident bank; DeviceAugmentor.apply on one seeded plan gives
    the same bytes with either bank"""
    import augment_cases as ac
    from btcdet_amd.device_augmentor import DataAugmentor, DeviceAugmentor, ObjectBank
    root, frames, dbs = built
    db = dbs["all_"]
    pkl = db.save(root)
    for name, data in _golden_files():
        assert (root / "gt_database" / name).read_bytes() == data, name
    with open(pkl, "rb") as f:
        infos = pickle.load(f)
    gr.assert_db_infos_equal(infos, gr.gold(), "all_")
    file_bank = ObjectBank(root, infos, 4)
    resident = db.bank.tensor(DEV).cpu().numpy()
    for path, (first, n) in file_bank.table.items():
        f1, n1 = db.bank.table[path]
        assert n == n1 and file_bank.rows[first:first + n].tobytes() == resident[f1:f1 + n1].tobytes(), path
    results = []
    for bank, src in ((db.bank, db.db_infos), (file_bank, infos)):
        aug = DataAugmentor(root, ac.augmentor_cfg("model_w2"), ac.CLASSES, db_infos={k: copy.deepcopy(src[k]) for k in ac.CLASSES})
        dev_aug = DeviceAugmentor(aug, bank)
        scenes = ac.scenes()
        np.random.seed(ac.SEED)
        plan = dev_aug.plan(scenes)
        assert plan.paste_rows > 0, "the plan pastes objects of the new database"
        pts = torch.from_numpy(np.concatenate([s["points"] for s in scenes])).to(DEV)
        offs = torch.from_numpy(np.cumsum([0] + [s["points"].shape[0] for s in scenes]).astype(np.int32)).to(DEV)
        res = dev_aug.apply(pts, offs, plan)
        results.append((res["points"].cpu().numpy(), res["pre_rot_points"].cpu().numpy(), res["scene_offsets"].cpu().numpy()))
    for a, b in zip(*results):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
