"""The three entry points of include/btcdet_hip_templates.h (csrc/template_match.hip) against the numpy restatement of that header
(template_ref.restate_*, itself held to the reference's own functions and to a float64 brute force by
tests/test_template_builder_cpu.py), bit for bit: out of btc_nn_sqdist, max_dist, the sel_occ words, chosen, tmpl_offsets, src and the
template rows.  Then TemplateBuilder.build over the golden classes against what the reference's functions recorded (selection exact,
coordinates within 1 float32 ulp), and the resident bank inside DeviceAugmentor.  The expectation is never the device code.

  sizes    segments of 0 / 1 / 63 / 64 / 65 / 255 / 256 / 257 rows, and one row either side of the kernels' tiles: 256 target rows per
           LDS tile of the nearest neighbour, 512 candidate rows per LDS tile and 1024 query rows per register pass of the matcher
  K        1, top_k, 9 (more than the 8 candidates of a workgroup), candidates padded with -1 at the end and in the middle
  bitmaps  nx * ny = 31 / 32 / 33 bits; rows on index nx / ny; a candidate wholly outside the object's box; rows exactly on a face
  greedy   the object among its own candidates, a winner that adds 4 rows and one that adds 5, an object of zero rows, a stop on
           num_extra_coords, three rounds (the reference's list index after a deletion), capacity below the total"""
import os

import numpy as np
import pytest
import torch

import template_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "templates.npz")
CLASSES = ("Car", "Cyclist", "Pedestrian")
SIZES = [0, 1, 63, 64, 65, 255, 256, 257]


def builder(**kw):
    from btcdet_amd.template_builder import TemplateBuilder
    return TemplateBuilder([], device=DEV, **kw)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _cloud(rng, n, scale=(2.0, 1.0, 0.8)):
    return (rng.uniform(-1, 1, (n, 3)) * np.array(scale)).astype(np.float32)


def _layout(sets):
    counts = np.array([s.shape[0] for s in sets], np.int64)
    seg = np.stack([np.cumsum(counts) - counts, counts], axis=1).astype(np.int32)
    pts = np.concatenate(sets, axis=0) if len(sets) else np.zeros((0, 3), np.float32)
    return _t(pts.reshape(-1, 3)), seg


@pytest.fixture(scope="module")
def golds():
    return {name: tr.load_golden(GOLD, name) for name in CLASSES}


# ---------------------------------------------------------------------------------------------------------------------- btc_nn_sqdist
def test_nn_sqdist_at_segment_and_tile_edges():
    rng = np.random.default_rng(5)
    sizes = SIZES + [511, 512, 513]
    q_sets, t_sets = [_cloud(rng, n) for n in sizes], [_cloud(rng, n) for n in sizes]
    q, q_seg = _layout(q_sets)
    t, t_seg = _layout(t_sets)
    pairs = np.array([[q_seg[a, 0], q_seg[a, 1], t_seg[b, 0], t_seg[b, 1]] for a in range(len(sizes)) for b in range(len(sizes))], np.int32)
    out = builder().nn_sqdist(q, t, pairs).cpu().numpy()
    want = np.concatenate([tr.nn_sqdist(q_sets[a], t_sets[b]) for a in range(len(sizes)) for b in range(len(sizes))])
    assert out.shape == want.shape and out.tobytes() == want.tobytes()
    assert np.isinf(want).any() and (want == 0).sum() == 0
    same = builder().nn_sqdist(q, q, np.array([[q_seg[5, 0], 255, q_seg[5, 0], 255]], np.int32)).cpu().numpy()   # a set against itself
    assert same.tobytes() == np.zeros((255,), np.float32).tobytes()
    assert builder().nn_sqdist(q, t, np.zeros((0, 4), np.int32)).shape == (0,)


# --------------------------------------------------------------------------------------------------------------- btc_match_candidates
def _match_case(rng, sizes, K, pad):
    sets = [_cloud(rng, n) for n in sizes]
    M = len(sets)
    halves = (rng.uniform(0.5, 1.0, (M, 3)) * np.array([2.0, 1.0, 0.8])).astype(np.float32)
    halves[1] = 1e-3                                                       # every candidate is wholly outside object 1's box
    for j in range(M):                                                     # rows exactly on a face of object 0's box, and just outside
        if sets[j].shape[0] >= 6:
            sets[j][0], sets[j][1], sets[j][2] = halves[0] * [1, 0.5, 0.5], halves[0] * [0.5, -1, 0.5], halves[0] * [-0.5, 0.5, 1]
            sets[j][3] = np.nextafter(halves[0], np.float32(9)) * [1, 0.5, 0.5]
    cand = np.stack([rng.permutation(M)[:K] if K <= M else rng.integers(0, M, K) for _ in range(M)]).astype(np.int32)
    cand[0, 0], cand[2, 0] = 0, 2                                           # the object among its own candidates
    if pad:
        cand[:, -1] = -1
        cand[3, K // 2] = -1
    return sets, halves, cand


@pytest.mark.parametrize("grid", [(31, 1), (4, 8), (3, 11), (25, 13)], ids=["31bits", "32bits", "33bits", "325bits"])
@pytest.mark.parametrize("K,pad", [(1, False), (3, False), (9, True)], ids=["K1", "K3", "K9pad"])
def test_match_candidates_bit_for_bit(grid, K, pad):
    rng = np.random.default_rng(100 * K + grid[0])
    sizes = SIZES + [511, 512, 513, 1023, 1024, 1025]
    sets, halves, cand = _match_case(rng, sizes, K, pad)
    nx, ny = grid
    g = dict(x0=np.float32(-2), y0=np.float32(-1), cell=np.float32(4.0 / nx), nx=nx, ny=ny)
    sets[4][5] = [-2 + 4.0, 0, 0]                                           # index nx exactly: no bit
    pts, seg = _layout(sets)
    M = len(sets)
    obj = np.arange(M, dtype=np.int32)
    md, so = builder().match(pts, _t(seg), _t(halves), M, _t(obj), _t(cand), g)
    want_md, want_so = tr.restate_match(sets, list(halves), obj, cand, g)
    md, so = md.cpu().numpy(), so.cpu().numpy().view(np.uint32)
    assert so.shape == want_so.shape and so.tobytes() == want_so.tobytes()
    assert md.tobytes() == want_md.tobytes()
    assert not want_so[1].any() and want_so[2:].any() and (want_md[0][cand[0] >= 0] == 0).all() and np.isinf(want_md[1:, 0][cand[1:, 0] == 0]).all()


def test_match_candidates_objects_outside_the_class_are_no_candidates():
    rng = np.random.default_rng(8)
    sets = [_cloud(rng, n) for n in (40, 70)]
    pts, seg = _layout(sets)
    g = dict(x0=np.float32(-2), y0=np.float32(-1), cell=np.float32(0.5), nx=8, ny=4)
    obj, cand = np.array([0, 7, -1, 1], np.int32), np.array([[1, 2], [0, 1], [0, 1], [-5, 0]], np.int32)
    half = np.full((2, 3), 3.0, np.float32)
    md, so = builder().match(pts, _t(seg), _t(half), 2, _t(obj), _t(cand), g)
    want_md, want_so = tr.restate_match(sets, list(half), obj, cand, g)
    assert md.cpu().numpy().tobytes() == want_md.tobytes() and so.cpu().numpy().view(np.uint32).tobytes() == want_so.tobytes()
    assert np.isinf(want_md[1:3]).all() and np.isfinite(want_md[0, 0]) and np.isinf(want_md[0, 1])


# --------------------------------------------------------------------------------------------------------------- btc_select_templates
def _select(tb, sets, halves, obj, cand, iou, grid, params, num_extra=2000, capacity=None):
    """match + select on the device and restated -> (device results, restated results), numpy"""
    pts, seg = _layout(sets)
    M = len(sets)
    d_seg = _t(seg)
    every = np.arange(M, dtype=np.int32)
    _, own = tb.match(pts, d_seg, torch.full((M, 3), float("inf"), device=DEV), M, _t(every), _t(every.reshape(M, 1)), grid)
    own = own.view(M, -1).contiguous()
    want_own = np.stack([tr.occ_words(s, grid) for s in sets])
    assert own.cpu().numpy().view(np.uint32).tobytes() == want_own.tobytes()
    md, so = tb.match(pts, d_seg, _t(np.stack(halves)), M, _t(obj), _t(cand), grid)
    want_md, want_so = tr.restate_match(sets, halves, obj, cand, grid)
    assert md.cpu().numpy().tobytes() == want_md.tobytes() and so.cpu().numpy().view(np.uint32).tobytes() == want_so.tobytes()
    tb.num_extra_coords = num_extra
    max_rows = int(seg[:, 1].max())
    want = tr.restate_select(sets, obj, cand, iou, want_md, want_so, want_own, params["max_num_bm"], num_extra, tb.iou_thresh,
                             params["ex_coords_ratio"], tr.nearest_sq(params["nearest_dist"]))
    cap = int(want[0][-1]) + 3 if capacity is None else capacity
    out, offs, chosen, src = tb.select(pts, d_seg, M, _t(obj), _t(cand), _t(iou), md, so, own, params, max_rows, cap, want_src=True)
    return (offs.astype(np.int32), chosen.cpu().numpy(), out.cpu().numpy(), src.cpu().numpy()), want


def _same_templates(got, want):
    assert got[0].tolist() == want[0].tolist(), "tmpl_offsets"
    assert got[1].tolist() == want[1].tolist(), "chosen"
    assert got[3].tobytes() == want[3].tobytes(), "src"
    assert got[2].tobytes() == want[2].tobytes(), "template rows"


@pytest.mark.parametrize("nbm", [1, 2, 3])
@pytest.mark.parametrize("name", CLASSES)
def test_select_templates_over_the_golden_classes(golds, name, nbm):
    """K = 5 with the object among its own candidates, a middle and a trailing -1, an object of zero rows; three rounds walk the
    reference's list index past two deletions"""
    gold = golds[name]
    sets = tr.golden_sets(gold, name)
    params = dict(tr.CLASS_PARAMS[name], max_num_bm=nbm)
    grid = tr.make_grid(sets)
    counts = np.array([tr.popcount(tr.occ_words(s, grid)) for s in sets])
    iou = tr.box_iou_origin(gold["boxes"][:, 3:6])
    cand, siou = tr.top_candidates(iou, counts > params["pnt_thresh"], 5)
    cand, siou = np.concatenate([cand, cand[:, :1]], axis=1), np.concatenate([siou, siou[:, :1]], axis=1)
    cand[:, -1] = -1
    cand[::3, 1] = -1
    obj = np.arange(len(sets), dtype=np.int32)
    got, want = _select(builder(), sets, [tr.half_dims(b) for b in gold["boxes"]], obj, cand, siou, grid, params)
    _same_templates(got, want)
    assert (want[1] >= 0).any() and min(s.shape[0] for s in sets) == 0
    if nbm == 3 and name == "Car":
        assert ((want[1] >= 0).sum(axis=1) >= 2).any()


def _four_or_five(extra_rows):
    """object 0 and a candidate that repeats its rows and brings `extra_rows` more, far from them, inside its box, in cells of their own"""
    rng = np.random.default_rng(3)
    own = (rng.uniform(-1, 1, (70, 3)) * [1.0, 0.5, 0.5]).astype(np.float32)
    far = np.array([[1.8 - 0.2 * k, 0.9, 0.0] for k in range(extra_rows)], np.float32)
    return [own, np.concatenate([own[::-1], far]), np.zeros((0, 3), np.float32)], [np.array([2.0, 1.0, 1.0], np.float32)] * 3


@pytest.mark.parametrize("extra_rows", [4, 5])
def test_a_winner_that_adds_four_rows_and_one_that_adds_five(extra_rows):
    sets, halves = _four_or_five(extra_rows)
    grid = tr.make_grid(sets)
    params = dict(mirror=False, pnt_thresh=0, ex_coords_ratio=5, max_num_bm=2, nearest_dist=0.05)
    obj, cand, iou = np.array([0, 2, 1], np.int32), np.array([[1], [1], [0]], np.int32), np.array([[0.95], [0.95], [0.5]], np.float32)
    got, want = _select(builder(), sets, halves, obj, cand, iou, grid, params)
    _same_templates(got, want)
    assert want[1][0].tolist() == ([1, -1] if extra_rows == 5 else [-1, -1])
    a = 5 if extra_rows == 5 else 0
    assert want[0].tolist() == [0, 70 + a, 70 + a + 70 + extra_rows, 70 + a + 2 * (70 + extra_rows)]
    # the empty object takes every row of its winner (IoU below the threshold does not stop an empty set); the low-IoU pair of object 1 stops


def test_a_stop_on_num_extra_coords_and_a_capacity_below_the_total(golds):
    gold = golds["Car"]
    sets = tr.golden_sets(gold, "Car")
    params = dict(tr.CLASS_PARAMS["Car"], max_num_bm=3)
    grid = tr.make_grid(sets)
    counts = np.array([tr.popcount(tr.occ_words(s, grid)) for s in sets])
    iou = tr.box_iou_origin(gold["boxes"][:, 3:6])
    cand, siou = tr.top_candidates(iou, counts > params["pnt_thresh"], 5)
    obj = np.arange(len(sets), dtype=np.int32)[::-1].copy()                 # a batch in another order than the class
    halves = [tr.half_dims(b) for b in gold["boxes"]]
    free, want_free = _select(builder(), sets, halves, obj, cand[::-1].copy(), siou[::-1].copy(), grid, params)
    _same_templates(free, want_free)
    stop = int(np.median([tr.popcount(tr.occ_words(s, grid)) for s in sets])) + 20
    got, want = _select(builder(), sets, halves, obj, cand[::-1].copy(), siou[::-1].copy(), grid, params, num_extra=stop)
    _same_templates(got, want)
    assert (want[1] >= 0).sum() < (want_free[1] >= 0).sum(), "the stop took rounds away"
    # capacity below the total: select() sees the larger total and calls again; the first call's outputs are checked through the ABI
    total = int(want_free[0][-1])
    again, _ = _select(builder(), sets, halves, obj, cand[::-1].copy(), siou[::-1].copy(), grid, params, capacity=total - 7)
    _same_templates(again, want_free)
    from btcdet_amd._lib import check, lib, ptr, stream_ptr, workspace
    tb = builder()
    pts, seg = _layout(sets)
    M, d_seg, d_obj, d_cand, d_iou = len(sets), _t(seg), _t(obj), _t(cand[::-1].copy()), _t(siou[::-1].copy())
    every = torch.arange(M, dtype=torch.int32, device=DEV)
    _, own = tb.match(pts, d_seg, torch.full((M, 3), float("inf"), device=DEV), M, every, every.view(M, 1).contiguous(), grid)
    md, so = tb.match(pts, d_seg, _t(np.stack(halves)), M, d_obj, d_cand, grid)
    cap, max_rows = total - 7, int(seg[:, 1].max())
    out = torch.full((total, 3), -7.0, device=DEV)
    src = torch.full((total, 2), -7, dtype=torch.int32, device=DEV)
    offs, chosen = torch.empty((M + 1,), dtype=torch.int32, device=DEV), torch.empty((M, 3), dtype=torch.int32, device=DEV)
    ws_bytes = lib().btc_select_templates_ws_bytes(M, 3, max_rows)
    ws = workspace(ws_bytes, DEV)
    check(lib().btc_select_templates(ptr(pts), pts.shape[0], ptr(d_seg), M, ptr(d_obj), ptr(d_cand), ptr(d_iou), ptr(md), ptr(so), ptr(own.view(M, -1)), M, 5,
                                     so.shape[2], 3, 2000, 0.90, 50.0, float(tr.nearest_sq(0.10)), max_rows, cap, ptr(out), ptr(src), ptr(offs), ptr(chosen),
                                     ptr(ws), ws_bytes, stream_ptr()), "btc_select_templates")
    assert offs.cpu().tolist() == want_free[0].tolist() and chosen.cpu().tolist() == want_free[1].tolist()
    assert out[:cap].cpu().numpy().tobytes() == want_free[2][:cap].tobytes() and src[:cap].cpu().numpy().tobytes() == want_free[3][:cap].tobytes()
    assert bool((out[cap:] == -7).all()) and bool((src[cap:] == -7).all()), "a row at or past the capacity was written"


# ------------------------------------------------------------------------------------------------------------------ TemplateBuilder
@pytest.mark.parametrize("top_k", [3, 5])
def test_build_equals_the_reference(golds, top_k):
    """the whole path -- two databases, the device rotation, the mirror, the project's box IoU, batches of 5 objects -- against what the
    reference's functions recorded: selection exact, coordinates within 1 ulp"""
    from btcdet_amd.template_builder import TemplateBuilder
    per_object = top_k * 9 * 4 + top_k * 12 + 12 * 16 + 2 * 500 * 13 + 500 * 12   # Car: 9 bitmap words, <= 12 eligible, 2 rounds, sets below 500 rows
    tb = TemplateBuilder(tr.golden_databases(golds), top_k=top_k, budget_bytes=5 * per_object, device=DEV)
    bank = tb.build(list(CLASSES))
    assert bank.tensor(DEV) is bank._resident and bank.nbytes == bank._resident.shape[0] * 12
    rows = bank.rows
    for name in CLASSES:
        gold, run = golds[name], golds[name]["runs"][top_k]
        print(name, top_k, tb.stats[name])
        assert name != "Car" or 5 <= tb.stats[name]["G"] < 12, "the Car class goes through in several batches"
        assert tb.chosen[name].tolist() == run["chosen"].tolist()
        for j, want in enumerate(run["templates"]):
            first, n = bank.table[(name, int(gold["image_idx"][j]), int(gold["gt_idx"][j]))]
            assert n == want.shape[0], (name, j)
            assert tr.ulp_apart(rows[first:first + n], want) <= 1, (name, j)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["device_route", "host_route"])
def test_the_bottom_cut_at_equality(dtype):
    """step 1 of build on the device: rows exactly on z = -dz/2 + bottom are cut, one float32 step above stays, one below goes; a
    float64 box (torch double on the GPU) and a float32 box (the host route), both bit for bit the restatement"""
    from btcdet_amd.template_builder import TemplateBuilder
    db, rows, boxes, keep = tr.bottom_database(dtype)
    tb = TemplateBuilder([db], device=DEV)
    kept, oid, counts = tb.normalized_sets(tb.class_objects("Car"))
    assert kept.device.type == torch.device(DEV).type
    want = [tr.restate_normalize(r, b) for r, b in zip(rows, boxes)]
    assert counts.tolist() == [int(keep.sum()), want[1].shape[0]] and kept.cpu().numpy().tobytes() == np.concatenate(want).tobytes()
    assert (rows[0][:, 2] == -boxes[0][5] / 2 + 0.15).sum() == 3 and int(keep.sum()) < rows[0].shape[0] - 5
    bank = tb.build(["Car"])                                     # and through build: every template starts with the cut, mirrored set
    for j, info in enumerate(tb.infos["Car"]):
        first, n = bank.table[("Car", int(info["image_idx"]), int(info["gt_idx"]))]
        own = tr.restate_mirror(want[j])
        assert n >= own.shape[0] and bank.rows[first:first + own.shape[0]].tobytes() == own.tobytes()


def _dx_iou(a, b):
    """a stand-in box IoU with many equal values: 0.95 where the first box is the longer one, else 0.92 (comparisons only: exact)"""
    return torch.where(a[:, 3].view(-1, 1) > b[:, 3].view(1, -1), 0.95, 0.92).to(torch.float32)


@pytest.mark.parametrize("name", ["Car", "Pedestrian"])
def test_equal_ious_take_the_lower_object_index(golds, name):
    """step 3 through build: with IoUs that tie, the candidates are the lower object indices first, and the whole result is the
    restatement's bit for bit"""
    from btcdet_amd.template_builder import TemplateBuilder
    gold = golds[name]
    tb = TemplateBuilder(tr.golden_databases({name: gold}), top_k=3, device=DEV)
    bank = tb.build([name], iou_fn=_dx_iou)
    dx = gold["boxes"][:, 3].astype(np.float32)
    iou = np.where(dx[:, None] > dx[None, :], np.float32(0.95), np.float32(0.92))
    sets = tr.golden_sets(gold, name)
    res = tr.restate_class(sets, gold["boxes"], tr.CLASS_PARAMS[name], 3, iou)
    ties = [np.diff(r) == 0 for r in res["iou"]]
    assert any(t.any() for t in ties) and all((np.diff(c)[t] > 0).all() for c, t in zip(res["cand"], ties)), "equal IoUs, ascending indices"
    assert tb.chosen[name].tolist() == res["chosen"].tolist()
    for j, want in enumerate(res["templates"]):
        first, n = bank.table[(name, int(gold["image_idx"][j]), int(gold["gt_idx"][j]))]
        assert n == want.shape[0] and bank.rows[first:first + n].tobytes() == want.tobytes(), (name, j)


def test_build_with_nothing_eligible_and_an_empty_class(golds):
    from btcdet_amd.template_builder import TemplateBuilder
    tb = TemplateBuilder(tr.golden_databases({"Pedestrian": golds["Pedestrian"]}), top_k=3, class_params={"Pedestrian": {"pnt_thresh": 10 ** 6}}, device=DEV)
    bank = tb.build(["Pedestrian", "Car"])
    sets = tr.golden_sets(golds["Pedestrian"], "Pedestrian")
    assert bank.rows.tobytes() == np.concatenate(sets).tobytes() and (tb.chosen["Pedestrian"] == -1).all() and tb.stats["Car"] == dict(objects=0)


def test_device_augmentor_takes_the_resident_bank(tmp_path):
    import augment_cases as ac
    import best_match_cases as bc
    from btcdet_amd.device_augmentor import DeviceAugmentor, TemplateBank
    results = []
    for kind in ("files", "resident"):            # a fresh augmentor each time: the sampler keeps its place between calls
        (tmp_path / kind).mkdir()
        aug, bank, arrays, roots = bc.build(tmp_path / kind, list(bc.ORDERS)[0])
        templates = TemplateBank(roots)
        if kind == "resident":
            templates = TemplateBank.from_rows(None, templates.table, device_rows=templates.tensor(DEV).clone())
            assert templates.tensor(DEV) is templates._resident
        dev_aug = DeviceAugmentor(aug, bank, templates=templates)
        scenes = bc.scenes()
        np.random.seed(ac.SEED)
        pts = torch.from_numpy(np.concatenate([s["points"] for s in scenes])).to(DEV)
        offs = torch.from_numpy(np.cumsum([0] + [s["points"].shape[0] for s in scenes]).astype(np.int32)).to(DEV)
        res = dev_aug.apply(pts, offs, dev_aug.plan(scenes), indexed_bm=True)
        results.append(res["special"]["bm_points"][0].cpu().numpy())
    assert results[0].shape[0] > 0 and results[0].tobytes() == results[1].tobytes()


def test_the_command_line_tool_on_a_kitti_directory(tmp_path):
    """KittiFrames -> GtDatabase.build -> TemplateBuilder.build -> save on the fixture directory of the ground-truth database tests: every
    template starts with the object's restated set (float64 boxes from the infos, rows from the resident ObjectBank), and the files
    read back as the bank that was built"""
    import sys
    import gt_database_ref as gr
    from btcdet_amd.device_augmentor import TemplateBank
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import create_templates
    root = gr.build_dir(gr.gold(), tmp_path)
    tb = create_templates.main([str(root), "--splits", "train", "--top-k", "3", "--device", DEV])
    assert tb.bank.tensor(DEV) is tb.bank._resident and sum(len(v) for v in tb.infos.values()) > 0
    db = tb.databases[0]
    for name in tb.built:
        assert all(i["box3d_lidar"].dtype == np.float64 for i in tb.infos[name])
        for info in tb.infos[name]:
            first, n = db.bank.table[info["path"]]
            kept = tr.restate_normalize(db.bank.rows[first:first + n], info["box3d_lidar"])
            want = tr.restate_mirror(kept) if tb.class_params[name]["mirror"] else kept
            f, m = tb.bank.table[(name, int(info["image_idx"]), int(info["gt_idx"]))]
            assert m >= want.shape[0] and tb.bank.rows[f:f + want.shape[0]].tobytes() == want.tobytes(), (name, info["path"])
    from btcdet_amd.template_builder import directory_name
    back = TemplateBank({name: str(tmp_path / directory_name(name, tb.class_params[name])) for name in tb.built})
    assert sorted(back.table) == sorted(tb.bank.table)
    for k, (f, m) in tb.bank.table.items():
        bf, bm = back.table[k]
        assert bm == m and back.rows[bf:bf + bm].tobytes() == tb.bank.rows[f:f + m].tobytes()
