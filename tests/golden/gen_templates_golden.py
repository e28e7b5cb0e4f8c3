"""Golden vectors of the reference's template maker (runs only where the reference is mounted): the REAL functions of
btcdet/datasets/multifindbestfit.py -- get_normalized_cloud, mirror, remove_voxelpnts, remove_outofbox, space_occ_voxelpnts, extra_occ,
get_batch_stats, find_best_match_boxpnts and find_multi_best_match_boxpnts -- imported through ref_env.install plus stubs of this
file's own for what that module imports and cannot have here: mayavi.mlab, visualize_utils, the chamfer extension (ChamferDistance as a
torch-CPU brute force with d2 = ((dx*dx) + (dy*dy)) + (dz*dz), no FMA), and torch.Tensor.to("cuda") as the identity.  The module's
__main__ is not a function and is not run: what it hands to find_best_match_boxpnts is formed here in this project's own words -- the
class extremes and grid, the eligible objects from the counts of the real space_occ_voxelpnts, the candidates by
template_ref.top_candidates (min(top_k, eligible) of them, where the script's topk would raise) over the box IoU its compiled op would
give, taken from the C oracle's restatement of iou3d_nms_kernel.cu (template_ref.box_iou_origin -> oracle.boxes_iou3d).

Data: per class of the script's table a seeded set of 12 objects of 0 - 300 rows (float64 boxes, float32 .bin rows), top_k 3 and 5.
The generator asserts margins, re-drawing the rows (or the class's boxes) that violate them, so that exact decisions are a fair demand
of a float32 restatement: every nearest distance the script thresholds is more than 1e-4 m from its threshold; every coordinate of
every set is more than 1e-4 m from a cell edge, from every object's box faces and from the bottom threshold; the smallest and second
smallest heuristic of every round differ by more than 1e-4; no two IoUs of a row are closer than 2e-4, none within that of 0.90.
Recorded per class: the inputs, and per top_k the template of every object as the script pickles it, the winner of every round that
appended rows (found by identity of the arrays handed to remove_voxelpnts) and the number of rows it appended.

    python tests/golden/gen_templates_golden.py   ->  tests/golden/templates.npz"""
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import oracle_spconv  # noqa: E402
import ref_env  # noqa: E402

ref_env.install(oracle_spconv)
import torch  # noqa: E402
import template_ref as tr  # noqa: E402

MARGIN, IOU_MARGIN = 1e-4, 2e-4      # the IoU margin is wider than the issue asks: the device op is held to its oracle within 1e-4
CLASSES = ("Car", "Cyclist", "Pedestrian")
TOP_KS = (3, 5)
M_OBJECTS = 12
BASE_DIMS = {"Car": (3.9, 1.6, 1.56), "Cyclist": (1.76, 0.6, 1.73), "Pedestrian": (0.8, 0.6, 1.73)}
SEEDS = {"Car": 11, "Cyclist": 12, "Pedestrian": 13}


class ChamferDistance(object):
    """dist1[b][i] = min_j d2(xyz1[b][i], xyz2[b][j]) (and the other side), float32, every operation rounded on its own"""

    def __call__(self, xyz1, xyz2):
        a, b = xyz1.float(), xyz2.float()
        d = a.unsqueeze(2) - b.unsqueeze(1)
        sq = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
        if sq.shape[2] == 0:
            return torch.full(sq.shape[:2], float("inf")), torch.zeros((sq.shape[0], 0))
        return sq.min(dim=2)[0], sq.min(dim=1)[0]


ref_env._mod("mayavi")
ref_env._mod("mayavi.mlab")
ref_env._mod("visualize_utils")
ref_env._mod("btcdet.ops.chamfer_distance", ChamferDistance=ChamferDistance)
_to = torch.Tensor.to
torch.Tensor.to = lambda self, *a, **k: self if (a and isinstance(a[0], str) and a[0].startswith("cuda")) else _to(self, *a, **k)

from btcdet.datasets import multifindbestfit as mf  # noqa: E402


class Violation(Exception):
    """rows index the object's file ("file"), its normalised rows ("kept") or its mirrored set ("set")"""

    def __init__(self, what, obj=None, rows=(), space="set"):
        Exception.__init__(self, what)
        self.what, self.obj, self.rows, self.space = what, obj, list(rows), space


LAST = {}      # the normalised rows and the sets of the run that raised


def file_rows(v, rows, boxes):
    """the rows of object v.obj's file behind a violation"""
    if v.space == "file":
        return sorted(set(int(r) for r in v.rows))
    keep = np.nonzero(rows[v.obj][:, 2].astype(np.float64) > (-boxes[v.obj, 5] / 2 + 0.15))[0]
    kept, out = LAST["kept"][v.obj], set()
    for r in v.rows:
        if v.space == "set" and r >= kept.shape[0]:          # a mirrored row: the kept row it is the image of
            r = int(np.argmin(np.abs(kept - LAST["sets"][v.obj][r] * np.array([1.0, -1.0, 1.0])).sum(axis=1)))
        out.add(int(keep[r]))
    return sorted(out)


# -------------------------------------------------------------------------------------------------------------------------- the data
def draw_boxes(rng, name):
    boxes = np.zeros((M_OBJECTS, 7), np.float64)
    boxes[:, 0:3] = rng.uniform([5, -20, -1.5], [60, 20, -0.5], (M_OBJECTS, 3))
    boxes[:, 3:6] = np.array(BASE_DIMS[name]) * (1 + rng.uniform(-0.035, 0.035, (M_OBJECTS, 3)))
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, M_OBJECTS)
    return boxes


def draw_rows(rng, box, n):
    """n rows of an object's .bin: points near the surface of its box, seen from one side, some outside the box and some under the
    bottom threshold, turned by +heading (the object files hold centred, unrotated-frame rows), x, y, z, intensity float32"""
    u = rng.normal(size=(n, 3))
    u /= np.maximum(np.abs(u).max(axis=1, keepdims=True), 1e-9)
    local = u * box[3:6] / 2 * rng.uniform(0.85, 1.04, (n, 1))
    c, s = np.cos(box[6]), np.sin(box[6])
    rows = np.stack([local[:, 0] * c - local[:, 1] * s, local[:, 0] * s + local[:, 1] * c, local[:, 2], rng.uniform(0, 1, n)], axis=1)
    return rows.astype(np.float32)


def draw_class(rng, name):
    boxes = draw_boxes(rng, name)
    sizes = [0, 1, 300] + [int(v) for v in rng.integers(3, 300, M_OBJECTS - 3)]
    order = rng.permutation(M_OBJECTS)
    rows = [None] * M_OBJECTS
    for j, n in zip(order, sizes):
        full = draw_rows(rng, boxes[j], 2 * n + 8)
        seen = full[(full[:, 0] * np.cos(boxes[j, 6] + 0.6) + full[:, 1] * np.sin(boxes[j, 6] + 0.6)) > rng.uniform(-1.0, 0.2)]
        rows[j] = np.ascontiguousarray(seen[:n])
    return boxes, rows


# ------------------------------------------------------------------------------------------------------- the script, function by function
def run_class(name, boxes, rows, top_k, tmp):
    """the script's __main__ for one class over files in `tmp` -> dict(templates, chosen, added, sets)"""
    P = tr.CLASS_PARAMS[name]
    cell = tr.COMMON["cell"]
    infos, origin_boxes, kept, sets = [], [], [], []
    LAST["kept"], LAST["sets"] = kept, sets
    for k, (obj_rows, box) in enumerate(zip(rows, boxes)):
        path = os.path.join(tmp, "%d.bin" % k)
        obj_rows.tofile(path)
        at_origin = np.zeros((7,), np.float64)                  # what the script matches with: the box's sides, no centre, no heading
        at_origin[3:6] = box[3:6]
        origin_boxes.append(at_origin)
        infos.append({"image_idx": "%06d" % (100 + k), "gt_idx": k % 4, "name": name})
        kept.append(mf.get_normalized_cloud(path, box, bottom=tr.COMMON["bottom"])[:, :3])
        if P["mirror"]:
            margin_mirror(kept[k], k)
        sets.append(mf.mirror(kept[k]) if P["mirror"] else kept[k])
    iou = tr.box_iou_origin(boxes[:, 3:6])                        # the script's compiled op, as the C oracle restates it
    full = [m for m in sets if m.shape[0]]
    lo, hi = np.min([m.min(axis=0) for m in full], axis=0), np.max([m.max(axis=0) for m in full], axis=0)
    allrange = np.concatenate([lo, hi])                           # float64, of the float64 sets the real functions work on
    nx, ny = (int(np.ceil((hi[a] - lo[a]) / cell)) for a in (0, 1))
    margin_sets(sets, boxes, allrange, cell)
    own = np.stack([mf.space_occ_voxelpnts(m, allrange, nx, ny, voxel_size=[cell] * 3) for m in sets])
    counts = own.reshape(len(sets), -1).sum(axis=1)
    eligible = counts > P["pnt_thresh"]
    margin_iou(iou[:, eligible])
    cand, cand_iou = tr.top_candidates(iou, eligible, top_k)     # descending, k = min(top_k, eligible); no ties inside the margin
    occ_map, coords_num = torch.from_numpy(own).to(torch.int32), torch.from_numpy(counts)
    sorted_iou, pnt_thresh_best_iou_indices = torch.from_numpy(cand_iou), torch.from_numpy(cand.astype(np.int64))
    all_db_infos_lst, box_dims_lst, pnts_lst, mirrored_pnts_lst, voxel_size = infos, origin_boxes, kept, sets, [cell] * 3
    ident = {id(m): j for j, m in enumerate(mirrored_pnts_lst)}
    M, nbm = len(rows), P["max_num_bm"]
    chosen, added, state, real = np.full((M, nbm), -1, np.int32), np.zeros((M, nbm), np.int32), {"car": -1, "calls": [0] * M}, mf.remove_voxelpnts

    def recording(sourcepnts, target_pnts, voxel_size=None, nearest_dist=None):
        """remove_voxelpnts as find_multi_best_match_boxpnts calls it: the set so far is the object's own array in its first round (and
        while nothing was appended), which names the object; the array of the winner names the winner"""
        state["car"] = ident.get(id(sourcepnts), state["car"])
        who, car = ident[id(target_pnts)], state["car"]
        dist = mf.cd_4pose(np.expand_dims(target_pnts[:, :3], axis=0), np.expand_dims(sourcepnts[:, :3], axis=0)).numpy()[0]
        near = np.nonzero(np.abs(dist.astype(np.float64) - nearest_dist) <= MARGIN)[0]
        if near.shape[0]:
            raise Violation("a greedy nearest distance within the margin", who, near)
        out = real(sourcepnts, target_pnts, nearest_dist=nearest_dist)
        r = state["calls"][car]
        state["calls"][car] += 1
        if out.shape[0] > 4:
            chosen[car, r], added[car, r] = who, out.shape[0]
        return out

    templates = []
    mf.remove_voxelpnts = recording
    try:
        with tempfile.TemporaryDirectory() as bm_dir:
            mf.find_best_match_boxpnts(all_db_infos_lst, box_dims_lst, sorted_iou, pnt_thresh_best_iou_indices, mirrored_pnts_lst, pnts_lst, coords_num,
                                       occ_map, bm_dir, allrange, nx, ny, voxel_size, max_num_bm=nbm, num_extra_coords=tr.COMMON["num_extra_coords"],
                                       iou_thresh=tr.COMMON["iou_thresh"], ex_coords_ratio=P["ex_coords_ratio"], nearest_dist=P["nearest_dist"],
                                       vis=False, save=True)
            for info in all_db_infos_lst:
                with open(os.path.join(bm_dir, str(int(info["image_idx"])) + "_" + str(int(info["gt_idx"])) + ".pkl"), "rb") as f:
                    templates.append(pickle.load(f))
    finally:
        mf.remove_voxelpnts = real
    return dict(templates=templates, chosen=chosen, added=added, sets=mirrored_pnts_lst, infos=all_db_infos_lst, allrange=allrange, nx=int(nx), ny=int(ny),
                cand=pnt_thresh_best_iou_indices.numpy(), iou=sorted_iou.numpy())


# ----------------------------------------------------------------------------------------------------------------------- the margins
def margin_mirror(car_pnts, obj):
    if car_pnts.shape[0] == 0:
        return
    flipped = car_pnts * np.array([1.0, -1.0, 1.0])
    d = np.sqrt(((flipped[:, None, :] - car_pnts[None, :, :]) ** 2).sum(-1)).min(axis=1)
    near = np.nonzero(np.abs(d - 0.05) <= MARGIN)[0]
    if near.shape[0]:
        raise Violation("a mirror nearest distance within the margin", obj, near, "kept")


def margin_sets(sets, boxes, allrange, cell):
    for j, m in enumerate(sets):
        if m.shape[0] == 0:
            continue
        bad = np.zeros((m.shape[0],), bool)
        for a in range(2):
            t = (m[:, a] - allrange[a]) / cell
            bad |= (np.abs(t - np.round(t)) * cell <= MARGIN) & (np.round(t) > 0)       # the class minimum sits on edge 0 exactly
        for b in boxes:
            bad |= (np.abs(np.abs(m) - b[3:6] * 0.5) <= MARGIN).any(axis=1)
        if bad.any():
            raise Violation("a coordinate within the margin of a cell edge or a box face", j, np.nonzero(bad)[0])


def margin_bottom(rows, boxes):
    for j, r in enumerate(rows):
        near = np.nonzero(np.abs(r[:, 2].astype(np.float64) - (-boxes[j, 5] / 2 + 0.15)) <= MARGIN)[0]
        if near.shape[0]:
            raise Violation("a row within the margin of the bottom threshold", j, near, "file")


def margin_iou(iou):
    for row in iou.astype(np.float64):
        s = np.sort(row)
        if (s.shape[0] > 1 and np.min(np.diff(s)) <= IOU_MARGIN) or np.any(np.abs(s - 0.90) <= IOU_MARGIN):
            raise Violation("two IoUs within the margin, or one of 0.90")


def margin_heuristic(name, boxes, sets32, top_k):
    audit = []
    tr.brute_class(sets32, boxes, tr.CLASS_PARAMS[name], top_k, tr.box_iou_origin(boxes[:, 3:6]), audit=audit)
    for obj, gap in audit:
        if gap is not None and gap <= MARGIN:
            raise Violation("the two smallest heuristics of a round within the margin")


def make_class(name):
    rng = np.random.default_rng(SEEDS[name])
    boxes, rows = draw_class(rng, name)
    for attempt in range(400):
        try:
            margin_bottom(rows, boxes)
            runs = {}
            for top_k in TOP_KS:
                with tempfile.TemporaryDirectory() as tmp:
                    runs[top_k] = run_class(name, boxes, rows, top_k, tmp)
                margin_heuristic(name, boxes, [s.astype(np.float32) for s in runs[top_k]["sets"]], top_k)
            print(name, "clean after", attempt, "re-draws")
            return boxes, rows, runs
        except Violation as v:
            if v.obj is None:
                print(name, attempt, v.what, "-> new boxes and rows")
                boxes, rows = draw_class(rng, name)
                continue
            todo = file_rows(v, rows, boxes)
            print(name, attempt, v.what, "object", v.obj, "file rows", todo[:8])
            for r in todo:
                rows[v.obj][r] = draw_rows(rng, boxes[v.obj], 1)[0]
    raise RuntimeError("no clean draw of class %s" % name)


if __name__ == "__main__":
    gold = {}
    for name in CLASSES:
        boxes, rows, runs = make_class(name)
        gold[name + "_boxes"] = boxes
        gold[name + "_rows"] = np.concatenate(rows, axis=0)
        gold[name + "_row_counts"] = np.array([r.shape[0] for r in rows], np.int32)
        infos = runs[TOP_KS[0]]["infos"]
        gold[name + "_image_idx"] = np.array([int(i["image_idx"]) for i in infos], np.int32)
        gold[name + "_gt_idx"] = np.array([int(i["gt_idx"]) for i in infos], np.int32)
        for top_k, run in runs.items():
            key = "%s_k%d_" % (name, top_k)
            assert all(t.dtype == np.float32 for t in run["templates"])
            gold[key + "templates"] = np.concatenate(run["templates"], axis=0)
            gold[key + "counts"] = np.array([t.shape[0] for t in run["templates"]], np.int32)
            gold[key + "set_counts"] = np.array([s.shape[0] for s in run["sets"]], np.int32)
            gold[key + "chosen"], gold[key + "added"] = run["chosen"], run["added"]
            gold[key + "cand"], gold[key + "iou"] = run["cand"].astype(np.int32), run["iou"].astype(np.float32)
            gold[key + "grid"] = np.array([run["allrange"][0], run["allrange"][1], run["nx"], run["ny"]], np.float64)
            print(key, "eligible", run["cand"].shape, "chosen", run["chosen"].T.tolist(), "rows", gold[key + "counts"].tolist())
    out = os.path.join(HERE, "templates.npz")
    np.savez_compressed(out, **gold)
    print("wrote", out, os.path.getsize(out), "bytes")
