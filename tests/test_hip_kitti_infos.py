"""btc_count_in_boxes and btc_coverage_cells (csrc/kitti_infos.hip, include/btcdet_hip_infos.h) against the numpy restatement of the header
(kitti_infos_ref.restate_counts / restate_jobs), exactly, at their edges; then end to end: KittiInfoBuilder.get_infos, add_coverage,
KittiEvaluator with coverage bins and create_kitti_infos over the raw synthetic directory, against what the reference's own functions
produced (tests/golden/kitti_infos.npz).

Counts: kernel and restatement form the same float32 operations, so any rows will do and none needs a margin.  Cells: the device's
atan2 may differ from numpy's in the last place, ~1e-13 of a cell; the designed rows sit at cell centres and the random ones are as far
from a cell edge as chance puts them (a few thousand values: a flip has a probability of ~1e-9)."""
import logging
import os
import pickle

import numpy as np
import pytest
import torch

import kitti_frames_ref as kr
import kitti_infos_ref as ir

pytestmark = pytest.mark.gpu
F32 = np.float32
CHUNK = 64            # IN_BOX_CHUNK of csrc/kitti_infos.hip
LDS_ROWS = 4096       # BTC_COVERAGE_LDS_KEYS / 2


# ------------------------------------------------------------------------------------------------------------------------ counts
def block_of(k):
    c = kr.parse_calib(kr.calib_text(kr.calib_arrays(k % 4)))
    H, W = kr.IMAGE_SHAPES[k % 4]
    return kr.calib_block(kr.lidar_to_rect_matrix(c["R0"], c["Tr_velo2cam"]), c["P2"], W, H)


def make_batch(sizes, nboxes, ld=4, seed=0):
    """scenes of `sizes` rows in front of and behind the camera, `nboxes` large boxes per scene among them"""
    rng = np.random.default_rng([77, seed])
    n = int(sum(sizes))
    pts = np.empty((n, ld), F32)
    pts[:, 0], pts[:, 1], pts[:, 2] = rng.uniform(-10, 40, n), rng.uniform(-15, 15, n), rng.uniform(-2, 1, n)
    pts[:, 3:] = rng.uniform(0, 1, (n, ld - 3))
    boxes = []
    for m in nboxes:
        boxes.append(np.stack([rng.uniform(2, 40, m), rng.uniform(-12, 12, m), rng.uniform(-1.5, 0.5, m), rng.uniform(4, 12, m), rng.uniform(3, 9, m),
                               rng.uniform(1.5, 3, m), rng.uniform(-3.1, 3.1, m)], axis=1).reshape(m, 7))
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    blocks = np.stack([block_of(s) for s in range(len(sizes))])
    return pts, offs, blocks, boxes


def device_points(pts, unaligned=False):
    flat = torch.empty((pts.size + 4,), dtype=torch.float32, device="cuda")
    view = flat[1:1 + pts.size] if unaligned else flat[:pts.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(pts).reshape(-1)))
    t = view.view(pts.shape)
    assert pts.size == 0 or t.data_ptr() % 16 == (4 if unaligned else 0)      # (a tensor of no element has no address to speak of)
    return t


def run_counts(pts, offs, blocks, boxes, unaligned=False, want_fov=True):
    from btcdet_amd.kitti_infos import count_in_boxes
    return count_in_boxes(device_points(pts, unaligned), offs, blocks, boxes, want_fov_rows=want_fov)


def check_counts(pts, offs, blocks, boxes, **kw):
    counts, fov = run_counts(pts, offs, blocks, boxes, **kw)
    want, want_fov = ir.restate_counts(pts, offs, blocks, boxes)
    print("rows", np.diff(offs).tolist(), "boxes", [b.shape[0] for b in boxes], "in view", want_fov.tolist(), "inside", int(want.sum()))
    assert counts.dtype == np.int32 and counts.tolist() == want.tolist()
    assert fov is None or fov.tolist() == want_fov.tolist()
    return want, want_fov


@pytest.mark.parametrize("sizes,nboxes", [((0,), (2,)), ((300,), (0,)), ((0, 0), (0, 0)), ((257, 0, 130), (3, 2, 0)), ((255,), (4,)), ((256,), (4,)),
                                          ((257,), (4,)), ((100, 100, 56), (2, 3, 1)), ((700, 1, 513), (5, 1, 7))],
                         ids=["n0", "m0", "n0m0", "empty_scene_and_no_boxes", "255", "256", "257", "boundary_in_256", "three_scenes"])
@pytest.mark.parametrize("layout", ["ld4", "ld5", "unaligned"])
def test_count_in_boxes_equals_the_restatement(sizes, nboxes, layout):
    pts, offs, blocks, boxes = make_batch(sizes, nboxes, ld=5 if layout == "ld5" else 4, seed=len(sizes))
    want, fov = check_counts(pts, offs, blocks, boxes, unaligned=layout == "unaligned")
    if sum(sizes) >= 255 and sum(nboxes):
        assert want.sum() > 0 and 0 < fov.sum() < sum(sizes), "a case that decides something"
    counts, none = run_counts(pts, offs, blocks, boxes, want_fov=False)            # fov_rows NULL
    assert none is None and counts.tolist() == want.tolist()


@pytest.mark.parametrize("m", [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5])
def test_count_in_boxes_at_the_lds_chunk(m):
    pts, offs, blocks, boxes = make_batch((300, 290), (m, 2), seed=m)
    boxes[0][-1] = [20.0, 0.0, -0.5, 30.0, 24.0, 3.0, 0.0]                            # the last box of the last chunk holds rows for certain
    want, _ = check_counts(pts, offs, blocks, boxes)
    assert want[m - 1] > 20 and np.count_nonzero(want[:m - 1]) > 0 and want[m:].sum() > 0


def test_count_in_boxes_decisions():
    pts, offs, blocks, boxes = make_batch((200, 60), (1, 1), seed=5)
    front = np.array([20.0, 0.0, -0.5, 10.0, 8.0, 3.0, 0.4])
    behind = np.array([-6.0, 0.0, -0.5, 8.0, 20.0, 3.0, 0.0])
    pts[190] = [np.nan, 0.0, -0.5, 0.5]                                              # a NaN row inside the first box's extent
    pts[191] = [20.0, np.nan, -0.5, 0.5]
    pts[200:, 0] += 100.0                                                            # scene 1's rows are far from every box
    boxes = [np.stack([front, front, behind]), front[None]]                          # scene 1's box lies over scene 0's rows
    want, fov = check_counts(pts, offs, blocks, boxes)
    inside = [int(ir.gr.restate_mask(pts[:200], row).sum()) for row in ir.hull_rows(boxes[0])]
    assert want[0] == want[1] > 0, "a row inside two boxes counts in both"
    assert inside[2] > 0 and want[2] == 0, "rows inside a box behind the camera are not seen"
    assert want[3] == 0 and inside[0] > 0, "a box counts the rows of its own scene only"
    assert want[0] <= inside[0] and fov[0] < 200


def test_count_in_boxes_bare_hull_has_no_margin():
    """heading 0, centre at the origin of x and y: lx = x exactly.  A row at x = dx / 2 is outside, its lower neighbour inside; the
    0.01-inflated test of btc_cut_objects would take both"""
    calib, shape, _, _ = kr.exact_case()
    block = kr.calib_block(kr.lidar_to_rect_matrix(calib["R0"], calib["Tr_velo2cam"]), calib["P2"], 4000, 4000)
    hx = F32(1.5)
    rows = [(hx, 0.0, 0.0), (np.nextafter(hx, F32(0)), 0.0, 0.0), (hx + F32(0.005), 0.0, 0.0), (1.0, 0.0, 0.25), (1.0, 0.0, np.nextafter(F32(0.25), F32(1)))]
    pts = np.array([list(r) + [0.5] for r in rows], F32)
    boxes = [np.array([[0.0, 0.0, 0.0, 3.0, 2.0, 0.5, 0.0]])]
    seen = kr.restate_keep(pts, block)
    want, fov = check_counts(pts, [0, len(rows)], block[None], boxes)
    assert seen.all() and fov[0] == len(rows) and want[0] == 2, (seen, want)


def test_fov_rows_are_the_rows_load_batch_keeps(tmp_path):
    from btcdet_amd.kitti_frames import KittiFrames
    from btcdet_amd.kitti_infos import KittiInfoBuilder, count_in_boxes
    root = ir.build_dir(ir.gold(), tmp_path)
    infos = KittiInfoBuilder(root, "train").get_infos(count_inside_pts=False)
    frames = KittiFrames(root, "train", infos=infos)
    idx = list(range(len(frames)))
    kept = frames.load_batch(idx, "cuda", crop=True)["scene_counts"]
    raw = frames.load_batch(idx, "cuda", crop=False)
    offs = np.concatenate([[0], np.cumsum(raw["raw_rows"])])
    _, fov = count_in_boxes(raw["points"], offs, frames.calib_blocks(idx), [x["annos"]["gt_boxes_lidar"] for x in infos])
    assert fov.tolist() == list(kept) and 0 < sum(kept) < offs[-1]


# ------------------------------------------------------------------------------------------------------------------------- cells
def sph(r, az, el):
    """a point with the given range and angles (degrees), float32"""
    a, e = np.deg2rad(az), np.deg2rad(el)
    return [r * np.cos(e) * np.cos(a), -r * np.cos(e) * np.sin(a), r * np.sin(e)]


IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0])


def run_jobs(tmpl, obj, jobs, pose, ld=4):
    from btcdet_amd.kitti_infos import coverage_cells
    tmpl = np.asarray(tmpl, F32).reshape(-1, 3)
    rows = np.zeros((np.asarray(obj).reshape(-1, 3).shape[0], ld), F32)
    rows[:, 0:3] = np.asarray(obj, F32).reshape(-1, 3)
    rows[:, 3:] = 0.25
    cells, status = coverage_cells(torch.from_numpy(tmpl).cuda(), torch.from_numpy(rows).cuda(), np.asarray(jobs, np.int32), np.asarray(pose, np.float64))
    want, want_status = ir.restate_jobs(tmpl, rows, jobs, np.asarray(pose, np.float64).reshape(-1, 5))
    assert status.tolist() == want_status.tolist() and cells.tolist() == want.tolist(), (cells.tolist(), want.tolist(), status.tolist())
    return cells, status


def random_object(rng, n_t, n_o, centre, yaw, extent=(4.0, 1.8, 1.6)):
    t = (rng.uniform(-0.55, 0.55, (n_t, 3)) * np.array(extent)).astype(F32)
    o = (rng.uniform(-0.5, 0.5, (n_o, 3)) * np.array(extent)).astype(F32)
    c, s = np.cos(yaw), np.sin(yaw)
    o = np.stack([o[:, 0] * c - o[:, 1] * s, o[:, 0] * s + o[:, 1] * c, o[:, 2]], axis=1).astype(F32)
    return t, o, np.array([centre[0], centre[1], centre[2], c, s])


def test_coverage_cells_no_job():
    cells, status = run_jobs(np.zeros((3, 3)), np.zeros((2, 3)), np.zeros((0, 4), np.int32), np.zeros((0, 5)))
    assert cells.shape == (0, 2) and status.shape == (0,)


def test_coverage_cells_kept_and_dropped_cells():
    """mn = 0 in every coordinate: the template's cells are (31, 10, 5) and (38, 39, 10), so n = (49, 50, 21)"""
    r, a, e = 0.32, 0.5184, 0.4203125
    tmpl = [sph(31.5 * r, 10.5 * a, 5.5 * e), sph(38.5 * r, 39.5 * a, 10.5 * e)]
    obj = [sph(48.5 * r, 10.5 * a, 5.5 * e),      # range cell max + 10: kept
           sph(49.5 * r, 10.5 * a, 5.5 * e),      # range cell max + 11: dropped
           sph(31.5 * r, 49.5 * a, 5.5 * e),      # azimuth cell max + 10: kept
           sph(31.5 * r, 50.5 * a, 5.5 * e),      # dropped
           sph(31.5 * r, 10.5 * a, 20.5 * e),     # elevation cell max + 10: kept
           sph(31.5 * r, 10.5 * a, 21.5 * e),     # dropped
           sph(31.5 * r, -0.5 * a, 5.5 * e),      # azimuth cell -1: dropped
           sph(31.5 * r, 10.5 * a, -0.5 * e),     # elevation cell -1: dropped
           sph(48.5 * r, 10.5 * a, 5.5 * e), sph(48.6 * r, 10.4 * a, 5.6 * e)]      # the first kept cell twice more
    cells, _ = run_jobs(tmpl, obj, [[0, 2, 0, len(obj)]], [IDENTITY])
    assert cells.tolist() == [[3, 2]]
    mn, _, _ = ir.restate_quotients(np.asarray(tmpl, F32), np.asarray(obj, F32), IDENTITY)
    assert mn.tolist() == [0.0, 0.0, 0.0]
    # the same template below the horizon and to the left: mn < 0 in both angles, and a cell below mn is dropped
    # (fractions .2 and .5 against minima at .5: no quotient lands on an integer)
    tmpl2 = [sph(31.5 * r, -10.2 * a, -5.2 * e), sph(38.5 * r, -39.5 * a, -10.5 * e)]      # cells (31, 29, 5), (38, 0, 0): n = (49, 40, 16)
    obj2 = [sph(31.5 * r, -20.2 * a, -7.2 * e),       # (31, 19, 3): kept
            sph(31.5 * r, -40.2 * a, -7.2 * e),       # azimuth below mn: dropped
            sph(31.5 * r, -20.2 * a, -11.2 * e),      # elevation below mn: dropped
            sph(31.5 * r, -0.2 * a, 3.2 * e)]         # (31, 39, 13): kept, azimuth cell n - 1
    cells, _ = run_jobs(tmpl2, obj2, [[0, 2, 0, 4]], [IDENTITY])
    mn, _, _ = ir.restate_quotients(np.asarray(tmpl2, F32), np.asarray(obj2, F32), IDENTITY)
    assert mn[0] == 0.0 and mn[1] < 0 and mn[2] < 0 and cells.tolist() == [[2, 2]]


def test_coverage_cells_small_templates_and_empty_objects():
    rng = np.random.default_rng(31)
    t, o, pose = random_object(rng, 40, 50, (15.0, 3.0, -0.8), 0.7)
    one = t[:1]
    dup = np.repeat(t[5:6], 33, axis=0)
    tmpl = np.concatenate([t, one, dup])
    jobs = [[0, 40, 0, 50], [0, 0, 0, 50], [40, 1, 0, 50], [41, 33, 0, 50], [0, 40, 0, 0], [40, 1, 50, 0], [0, 0, 0, 0]]
    cells, status = run_jobs(tmpl, o, jobs, [pose] * len(jobs))
    assert status.tolist() == [0] * len(jobs)
    assert cells[1].tolist() == [0, 0] and cells[6].tolist() == [0, 0], "a template of no row"
    assert cells[2, 1] == 1 and cells[3, 1] == 1 and cells[0, 1] > 20, "one row, 33 equal rows, 40 rows"
    assert cells[4, 0] == 0 and cells[4, 1] == cells[0, 1] and cells[5].tolist() == [0, 1], "an object of no row"
    assert cells[0, 0] > 10


def test_coverage_cells_behind_the_sensor_across_the_seam():
    rng = np.random.default_rng(32)
    t, o, pose = random_object(rng, 300, 200, (-20.0, 0.05, -1.2), 2.9)
    st = ir.restate_template_sphere(t, pose)
    assert st[:, 1].min() < -175 and st[:, 1].max() > 175, "the template's azimuths lie on both sides of the seam"
    cells, _ = run_jobs(t, o, [[0, 300, 0, 200]], [pose])
    mn, qt, _ = ir.restate_quotients(t, o, pose)
    assert mn[1] < -175 and mn[2] < 0 and np.floor(qt[:, 1]).max() + 11 <= 705 and cells[0, 1] > 100


def test_coverage_cells_set_exactly_half_full():
    """64 template rows give a table of 128 slots; 64 distinct keys fill exactly half of it"""
    tmpl = [sph((5.5 + i) * 0.32, 10.5 * 0.5184, 5.5 * 0.4203125) for i in range(64)]
    obj = [sph((5.5 + i) * 0.32, 10.5 * 0.5184, 5.5 * 0.4203125) for i in range(64)][::-1]
    cells, _ = run_jobs(tmpl, obj, [[0, 64, 0, 64]], [IDENTITY])
    assert cells.tolist() == [[64, 64]]


@pytest.mark.parametrize("rows", [LDS_ROWS - 1, LDS_ROWS, LDS_ROWS + 1])
@pytest.mark.parametrize("ld", [4, 3])
def test_coverage_cells_at_the_lds_limit(rows, ld):
    """LDS_ROWS + 1 rows need a table of 16384 keys: the workspace path.  The other job of the call stays small."""
    from btcdet_amd import _lib
    rng = np.random.default_rng(rows)
    t, o, pose = random_object(rng, rows, rows, (25.0, -6.0, -0.5), -1.1, extent=(30.0, 20.0, 6.0))
    t2, o2, pose2 = random_object(rng, 50, 40, (12.0, 2.0, -0.7), 0.3)
    jobs = [[0, rows, 0, rows], [rows, 50, rows, 40]]
    cells, _ = run_jobs(np.concatenate([t, t2]), np.concatenate([o, o2]), jobs, [pose, pose2], ld=ld)
    assert cells[0, 1] > rows // 4 and cells[0, 0] > rows // 8 and cells[1, 1] > 20
    assert (_lib.lib().btc_coverage_cells_ws_bytes(1, rows) > 256) == (rows > LDS_ROWS)


def test_coverage_cells_many_jobs():
    rng = np.random.default_rng(33)
    tmpl, obj, jobs, pose, t_at, o_at = [], [], [], [], 0, 0
    for j in range(150):
        n_t, n_o = int(rng.integers(0, 220)), int(rng.integers(0, 180))
        centre = (rng.uniform(-30, 60), rng.uniform(-30, 30), rng.uniform(-1.5, 0.5))
        if np.hypot(centre[0], centre[1]) < 4:
            centre = (centre[0] + 8, centre[1], centre[2])
        t, o, p = random_object(rng, n_t, n_o, centre, rng.uniform(-3.1, 3.1))
        tmpl.append(t), obj.append(o), pose.append(p), jobs.append([t_at, n_t, o_at, n_o])
        t_at, o_at = t_at + n_t, o_at + n_o
    cells, status = run_jobs(np.concatenate(tmpl), np.concatenate(obj), jobs, pose)
    assert not status.any() and np.count_nonzero(cells[:, 0]) > 100
    again, _ = run_jobs(np.concatenate(tmpl), np.concatenate(obj), jobs[::-1], pose[::-1])
    assert again[::-1].tolist() == cells.tolist(), "a job's result does not depend on its place in the table"


def test_coverage_cells_wide_job_goes_to_the_host(caplog):
    from btcdet_amd.device_augmentor import ObjectBank, TemplateBank
    from btcdet_amd.kitti_infos import add_coverage, coverage_cells_host
    rng = np.random.default_rng(34)
    box = np.array([330.0, 4.0, -1.0, 4.0, 1.8, 1.6, 0.4])                            # past 327.68 m: 1024 range cells
    t, o, pose = random_object(rng, 120, 90, box[:3], box[6])
    near = pose.copy()
    near[0] = 300.0
    cells, status = run_jobs(np.concatenate([t, t]), np.concatenate([o, o]), [[0, 120, 0, 90], [120, 120, 90, 90]], [pose, near])
    assert status.tolist() == [1, 0] and cells[0].tolist() == [0, 0] and cells[1, 1] > 5      # (a car at 300 m spans few cells)
    uo, ub, st = ir.restate_cells(t, o, pose, limit=None)
    assert st == 0 and coverage_cells_host(t, o, box) == (uo, ub) and ub > 5
    infos = [{"point_cloud": {"lidar_idx": "000001"}, "annos": {"name": np.array(["Car"]), "gt_boxes_lidar": box[None]}}]
    rows = np.concatenate([o, np.full((o.shape[0], 1), 0.5, F32)], axis=1)
    bank = ObjectBank.from_rows(rows, {"gt_database/000001_Car_0.bin": (0, rows.shape[0])}, 4)
    with caplog.at_level(logging.WARNING, logger="btcdet_amd.kitti_infos"):
        add_coverage(infos, bank, TemplateBank.from_arrays({("Car", 1, 0): t}), "train")
    got = infos[0]["annos"]["coverage_rates"]
    assert got.shape == (1, 1) and got[0, 0] == uo / max(1, ub) and "counted on the host" in caplog.text


# -------------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def raw_dir(tmp_path_factory):
    return ir.build_dir(ir.gold(), tmp_path_factory.mktemp("kitti_raw"))


@pytest.fixture(scope="module")
def built_infos(raw_dir):
    from btcdet_amd.kitti_infos import KittiInfoBuilder
    return KittiInfoBuilder(raw_dir, "train").get_infos(frames_per_batch=2)


def test_get_infos_equals_the_reference(raw_dir, built_infos):
    from btcdet_amd.kitti_infos import KittiInfoBuilder
    g = ir.gold()
    ir.assert_infos_equal(built_infos, g, "info", n_frames=ir.N_FRAMES)
    for k, info in enumerate(built_infos):
        print("frame", k, "num_points_in_gt", info["annos"]["num_points_in_gt"].tolist())
    one_batch = KittiInfoBuilder(raw_dir, "train").get_infos()
    ir.assert_infos_equal(one_batch, g, "info", n_frames=ir.N_FRAMES)
    some = KittiInfoBuilder(raw_dir, "train").get_infos(sample_id_list=["000042", "000003"], frames_per_batch=1)
    ir.assert_infos_equal(some, g, "info", frame_map=[3, 0])


@pytest.fixture(scope="module")
def covered(raw_dir, built_infos):
    import copy
    from btcdet_amd.device_augmentor import TemplateBank
    from btcdet_amd.gt_database import GtDatabase
    from btcdet_amd.kitti_frames import KittiFrames
    from btcdet_amd.kitti_infos import add_coverage
    infos = copy.deepcopy(built_infos)
    frames = KittiFrames(raw_dir, "train", fov_points_only=False, infos=infos)
    db = GtDatabase.build(frames, frames_per_batch=3)
    return add_coverage(infos, db.bank, TemplateBank.from_arrays(ir.template_arrays(ir.gold())), "train"), frames


def test_add_coverage_equals_the_reference(covered):
    g = ir.gold()
    for k, info in enumerate(covered[0]):
        got, want = info["annos"]["coverage_rates"], g["cov%d" % k]
        print("frame", k, "coverage_rates", got.reshape(-1).tolist())
        assert list(info["annos"].keys())[-1] == "coverage_rates"
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (k, got, want)


def test_evaluator_takes_the_coverage_bins(covered, built_infos):
    from btcdet_amd.kitti_eval import KittiEvaluator
    infos, frames = covered
    names = ["Car", "Pedestrian", "Cyclist"]
    bins = [[0.0, 0.3], [0.3, 0.7], [0.7, 100.0]]

    def evaluator(gt):
        ev = KittiEvaluator(gt, names, coverage_rates=bins)
        for i, info in enumerate(infos):
            a = info["annos"]
            keep = [j for j in range(a["gt_boxes_lidar"].shape[0]) if a["name"][j] in names]
            pred = {"pred_boxes": torch.from_numpy(a["gt_boxes_lidar"][keep].astype(F32)), "pred_scores": torch.full((len(keep),), 0.9),
                    "pred_labels": torch.tensor([names.index(a["name"][j]) + 1 for j in keep], dtype=torch.int64)}
            ev.add([frames.frame_id(i)], [pred], [frames.calib(i)], [frames.image_shape(i)])
        return ev

    text, ret, _ = evaluator([x["annos"] for x in infos]).result()
    assert isinstance(text, str) and "Car" in text and len(ret) > 0
    with pytest.raises(KeyError, match="coverage_rates"):                       # the infos as get_infos leaves them
        evaluator([x["annos"] for x in built_infos]).result()


def test_create_kitti_infos_from_a_raw_directory(tmp_path):
    from btcdet_amd.device_augmentor import TemplateBank
    from btcdet_amd.gt_database import GtDatabase
    from btcdet_amd.kitti_frames import KittiFrames
    from btcdet_amd.kitti_infos import create_kitti_infos, create_kitti_infos_with_coverage
    g = ir.gold()
    root = ir.build_dir(g, tmp_path, splits={"train": [0, 1, 2], "val": [3, 4]}, test_frames=[1, 3])
    assert not [f for f in os.listdir(root) if f.endswith(".pkl")]
    paths = create_kitti_infos(root, frames_per_batch=2)
    loaded = {s: pickle.load(open(p, "rb")) for s, p in paths.items()}
    ir.assert_infos_equal(loaded["train"], g, "info", n_frames=3, frame_map=[0, 1, 2])
    ir.assert_infos_equal(loaded["val"], g, "info", n_frames=2, frame_map=[3, 4])
    ir.assert_infos_equal(loaded["test"], g, "test", n_frames=2, frame_map=[1, 3])
    for split, folder in (("train", "gt_database"), ("val", "gt_database_val")):
        frames = KittiFrames(root, split, fov_points_only=False)                 # reads the pickle that was just written
        db = GtDatabase.build(frames)
        with open(os.path.join(root, "kitti_dbinfos_%s.pkl" % split), "rb") as f:
            saved = pickle.load(f)
        assert list(saved.keys()) == list(db.db_infos.keys()) and [e["num_points_in_gt"] for v in saved.values() for e in v] == \
            [e["num_points_in_gt"] for v in db.db_infos.values() for e in v]
        assert sorted(os.listdir(os.path.join(root, folder))) == sorted(os.path.basename(p) for p, _, _ in db.objects)
    cov = create_kitti_infos_with_coverage(root, TemplateBank.from_arrays(ir.template_arrays(g)))
    for split, ks in (("train", [0, 1, 2]), ("val", [3, 4])):
        infos = pickle.load(open(cov[split], "rb"))
        assert os.path.basename(str(cov[split])) == "kitti_cvrg_infos_%s.pkl" % split
        for info, k in zip(infos, ks):
            assert np.array_equal(info["annos"]["coverage_rates"], g["cov%d" % k]) and info["annos"]["coverage_rates"].shape == g["cov%d" % k].shape
