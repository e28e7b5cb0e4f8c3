"""numpy restatement of include/btcdet_hip_templates.h and of the host stages of btcdet_amd/template_builder.py, one float32 operation
per rounded step (restate_*), and a plain float64 brute force of the same algorithm written the way the reference's
multifindbestfit.py words it -- lists, deletion of the winner, sets of cells (brute_*).  The two are compared on decisions in
tests/test_template_builder_cpu.py; the kernels are held to restate_* bit for bit in tests/test_hip_template_match.py."""
import numpy as np

F = np.float32
INF = F(np.inf)

CLASS_PARAMS = {      # the reference's __main__ table
    "Car": dict(mirror=True, pnt_thresh=80, ex_coords_ratio=50, max_num_bm=2, nearest_dist=0.10),
    "Cyclist": dict(mirror=True, pnt_thresh=5, ex_coords_ratio=5, max_num_bm=1, nearest_dist=0.05),
    "Pedestrian": dict(mirror=False, pnt_thresh=5, ex_coords_ratio=5, max_num_bm=1, nearest_dist=0.05),
}
COMMON = dict(iou_thresh=0.90, num_extra_coords=2000, cell=0.16, bottom=0.15, mirror_dist=0.05)


# ------------------------------------------------------------------------------------------------------------------- float32 restatement
def d2(p, q):
    """(a, 3) x (b, 3) float32 -> (a, b): ((dx*dx) + (dy*dy)) + (dz*dz), every step rounded to float32"""
    p, q = np.asarray(p, F).reshape(-1, 1, 3), np.asarray(q, F).reshape(1, -1, 3)
    d = p - q
    return ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])


def nn_sqdist(q, t, chunk=512):
    """the smallest d2 of every row of q against t; +inf for an empty t"""
    q, t = np.asarray(q, F).reshape(-1, 3), np.asarray(t, F).reshape(-1, 3)
    out = np.full((q.shape[0],), INF, F)
    if t.shape[0]:
        for a in range(0, q.shape[0], chunk):
            out[a:a + chunk] = d2(q[a:a + chunk], t).min(axis=1)
    return out


def nearest_sq(nearest_dist):
    """the largest float32 whose correctly rounded square root is <= float32(nearest_dist)"""
    nd = F(nearest_dist)
    t = F(nd * nd)
    while np.sqrt(t) <= nd:
        t = np.nextafter(t, INF)
    while np.sqrt(t) > nd:
        t = np.nextafter(t, F(0))
    return t


def restate_normalize(rows, box, bottom=0.15):
    """step 1: x*c - y*s, x*s + y*c with c, s = cos, sin(-heading) in the box's dtype under numpy's promotion of the float32 rows with
    it (a float64 box: double, one rounding; a float32 box: float32 throughout); rows with z > -dz/2 + bottom, compared the same way"""
    p, box = np.asarray(rows, F)[:, :3], np.asarray(box)
    c, s = np.cos(-box[6]), np.sin(-box[6])
    x = p[:, 0] * c - p[:, 1] * s
    y = p[:, 0] * s + p[:, 1] * c
    keep = p[:, 2] > (-box[5] / 2 + bottom)
    return np.stack([x, y, p[:, 2]], axis=1)[keep].astype(F)


def bottom_case(dtype, bottom=0.15, seed=4):
    """an object whose rows sit exactly on z = -dz/2 + bottom, one float32 step above and one below (that comparison is exact, so
    these rows are exempt from the margins) -> (rows (n, 4) f32, box (7) of `dtype`, keep (n) bool: only the rows above stay).
    For a float64 box dz is searched so that the double threshold IS a float32 number."""
    rng = np.random.default_rng(seed)
    if dtype == np.float64:
        z0 = F(-0.6)
        while True:
            dz = 2.0 * (bottom - float(z0))
            if -dz / 2 + bottom == float(z0):
                break
            z0 = np.nextafter(z0, F(-1))
        thr = z0
    else:
        dz = F(1.5)
        thr = -dz / 2 + bottom
        assert isinstance(thr, np.floating) and thr.dtype == F
    box = np.array([10.0, 3.0, -1.0, 3.9, 1.6, float(dz), 0.7], dtype)
    assert F(-box[5] / 2 + bottom) == -box[5] / 2 + bottom == thr
    z = np.concatenate([[thr] * 3, [np.nextafter(thr, F(1))] * 3, [np.nextafter(thr, F(-1))] * 3, rng.uniform(-0.7, 0.7, 40)]).astype(F)
    order = rng.permutation(z.shape[0])
    rows = np.concatenate([rng.uniform(-1.5, 1.5, (z.shape[0], 2)), z[:, None], rng.uniform(0, 1, (z.shape[0], 1))], axis=1).astype(F)[order]
    keep = rows[:, 2].astype(np.float64) > float(thr)
    assert (rows[:, 2] == thr).sum() == 3 and 3 <= keep.sum() <= keep.shape[0] - 6
    return rows, box, keep


def bottom_database(dtype):
    """the case above as the one Car of a database, behind a second Car of the other kind of rows"""
    rows, box, keep = bottom_case(dtype)
    other = np.ascontiguousarray(rows[::-1] * F(0.5))
    infos = [{"name": "Car", "path": "a.bin", "image_idx": "000007", "gt_idx": 0, "box3d_lidar": box},
             {"name": "Car", "path": "b.bin", "image_idx": "000007", "gt_idx": 1, "box3d_lidar": box * np.array([1, 1, 1, 1, 1, 1, -1], dtype)}]
    table = {"a.bin": (0, rows.shape[0]), "b.bin": (rows.shape[0], other.shape[0])}
    return FakeDatabase({"Car": infos}, FakeBank(np.concatenate([rows, other]), table)), [rows, other], [i["box3d_lidar"] for i in infos], keep


def restate_mirror(kept, mirror_dist=0.05):
    kept = np.asarray(kept, F).reshape(-1, 3)
    flipped = kept * np.array([1, -1, 1], F)
    far = nn_sqdist(flipped, kept) > nearest_sq(mirror_dist)
    return np.concatenate([kept, flipped[far]], axis=0)


def half_dims(box):
    return (np.asarray(box, np.float64)[3:6] / 2).astype(F)


def make_grid(sets, cell=0.16):
    """x0, y0 (float32 minima over the non-empty sets), cell float32, nx, ny = ceil(extent / cell) in double"""
    full = [s for s in sets if s.shape[0]]
    if not full:
        return dict(x0=F(0), y0=F(0), cell=F(cell), nx=1, ny=1)
    lo = np.min([s.min(axis=0) for s in full], axis=0)
    hi = np.max([s.max(axis=0) for s in full], axis=0)
    nx = max(int(np.ceil((float(hi[0]) - float(lo[0])) / cell)), 1)
    ny = max(int(np.ceil((float(hi[1]) - float(lo[1])) / cell)), 1)
    return dict(x0=F(lo[0]), y0=F(lo[1]), cell=F(cell), nx=nx, ny=ny)


def grid_words(grid):
    return (grid["nx"] * grid["ny"] + 31) // 32


def occ_words(points, grid):
    points = np.asarray(points, F).reshape(-1, 3)
    words = np.zeros((grid_words(grid),), np.uint32)
    fx = np.floor((points[:, 0] - grid["x0"]) / grid["cell"])
    fy = np.floor((points[:, 1] - grid["y0"]) / grid["cell"])
    ok = (fx >= 0) & (fx < grid["nx"]) & (fy >= 0) & (fy < grid["ny"])
    b = fx[ok].astype(np.int64) * grid["ny"] + fy[ok].astype(np.int64)
    np.bitwise_or.at(words, b >> 5, (np.uint32(1) << (b & 31).astype(np.uint32)))
    return words


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8)).sum())


def restate_match(sets, halves, obj, cand, grid):
    """btc_match_candidates: obj (G), cand (G, K) -> max_dist (G, K) f32, sel_occ (G, K, W) u32"""
    G, K = cand.shape
    W, M = grid_words(grid), len(sets)
    md, so = np.full((G, K), INF, F), np.zeros((G, K, W), np.uint32)
    for g in range(G):
        i = int(obj[g])
        if not 0 <= i < M:
            continue
        for k in range(K):
            c = int(cand[g, k])
            if not 0 <= c < M:
                continue
            m = nn_sqdist(sets[i], sets[c])
            md[g, k] = np.sqrt(m.max()) if m.shape[0] else F(0)
            inside = np.all(np.abs(sets[c]) <= halves[i][None, :], axis=1)
            so[g, k] = occ_words(sets[c][inside], grid)
    return md, so


def restate_select_one(sets, i, cand, iou, md, so, own, max_num_bm, num_extra_coords, iou_thresh, ratio, nsq):
    """one object of btc_select_templates -> chosen (max_num_bm), list of (source object, kept row indices) segments"""
    M = len(sets)
    chosen = np.full((max_num_bm,), -1, np.int32)
    if not 0 <= i < M:
        return chosen, []
    segs = [(i, np.arange(sets[i].shape[0]))]
    alive = [(0 <= int(c) < M) for c in cand]
    aug, aug_num = own.copy(), 0
    ratio, iou_thresh = F(ratio), F(iou_thresh)
    for rnd in range(max_num_bm):
        if not any(alive):
            break
        best = None
        for k in range(len(cand)):
            if not alive[k]:
                continue
            extra = popcount(so[k] & ~aug)
            with np.errstate(divide="ignore"):
                h = F(F(F(md[k] + F(ratio / F(extra))) + F(2.0 if iou[k] < iou_thresh else 0.0)) + F(1.0 if extra < 30 else 0.0))
            if h == h and (best is None or h < best[0]):
                best = (h, k, extra)
        if best is None:
            break
        _, w, extra = best
        have = sum(len(r) for _, r in segs)
        if (iou[w] < iou_thresh and have > 0) or extra == 0:
            break
        listed = [k for k in range(len(cand)) if 0 <= int(cand[k]) < M]              # the reference's list of point sets: never shortened
        c = int(cand[listed[sum(alive[:w])]])                                          # ... and indexed with w's rank among the alive
        cur = np.concatenate([sets[j][r] for j, r in segs], axis=0)
        keep = np.nonzero(nn_sqdist(sets[c], cur) > nsq)[0]
        if keep.shape[0] > 4:
            segs.append((c, keep))
            chosen[rnd] = c
            aug = aug | so[w]
            aug_num = popcount(aug)
        if sum(alive) == 1 or aug_num >= num_extra_coords:
            break
        alive[w] = False
    return chosen, segs


def restate_select(sets, obj, cand, iou, md, so, own_occ, max_num_bm, num_extra_coords, iou_thresh, ratio, nsq):
    """btc_select_templates -> tmpl_offsets (G+1) i32, chosen (G, max_num_bm) i32, out (total, 3) f32, src (total, 2) i32"""
    G = len(obj)
    offs, chosen, out, src = [0], [], [], []
    for g in range(G):
        i = int(obj[g])
        ch, segs = restate_select_one(sets, i, cand[g], iou[g], md[g], so[g], own_occ[i] if 0 <= i < len(sets) else None, max_num_bm,
                                      num_extra_coords, iou_thresh, ratio, nsq)
        chosen.append(ch)
        for j, r in segs:
            out.append(sets[j][r])
            src.append(np.stack([np.full(len(r), j), r], axis=1))
        offs.append(offs[-1] + sum(len(r) for _, r in segs))
    cat = lambda parts, w, dt: np.concatenate(parts, axis=0).astype(dt) if parts else np.zeros((0, w), dt)
    return np.array(offs, np.int32), np.array(chosen, np.int32).reshape(G, max_num_bm), cat(out, 3, F), cat(src, 2, np.int32)


def box_iou_origin(dims):
    """the 3-D IoU of the boxes [0, 0, 0, dx, dy, dz, 0], all against all, float32, as the reference's compiled op gives it: the C
    oracle's restatement of iou3d_nms_kernel.cu (oracle.boxes_iou3d), the expectation the project's boxes_iou3d_gpu is tested against.
    For boxes that share a centre and an axis the rotated-polygon intersection of that kernel does NOT always return the product of the
    smaller sides (edges that run along each other); the templates the reference made carry what it returns, so this does too"""
    from oracle import oracle as orc
    d = np.asarray(dims, F).reshape(-1, 3)
    boxes = np.zeros((d.shape[0], 7), F)
    boxes[:, 3:6] = d
    return orc.boxes_iou3d(boxes, boxes)


def top_candidates(iou, eligible, top_k):
    """per row the top_k eligible columns by IoU, equal IoUs by lower index -> cand (M, K) i32, sorted iou (M, K) f32, K =
    min(top_k, number eligible); K == 0 when nothing is eligible"""
    cols = np.nonzero(eligible)[0]
    K = min(int(top_k), cols.shape[0])
    sub = iou[:, cols]
    order = np.argsort(-sub, axis=1, kind="stable")[:, :K]
    return cols[order].astype(np.int32), np.take_along_axis(sub, order, axis=1).astype(F)


def restate_class(sets, boxes, params, top_k, iou=None, common=COMMON):
    """steps 3-6 over the mirrored sets of a class -> dict(templates list, chosen (M, max_num_bm), segs, grid, cand, iou, counts)"""
    M = len(sets)
    grid = make_grid(sets, common["cell"])
    own = np.stack([occ_words(s, grid) for s in sets]) if M else np.zeros((0, grid_words(grid)), np.uint32)
    counts = np.array([popcount(w) for w in own], np.int64)
    if iou is None:
        iou = box_iou_origin(np.asarray(boxes, np.float64)[:, 3:6].astype(F))
    cand, siou = top_candidates(iou, counts > params["pnt_thresh"], top_k)
    halves = [half_dims(b) for b in boxes]
    nbm = params["max_num_bm"]
    res = dict(grid=grid, cand=cand, iou=siou, counts=counts, own=own, templates=[], chosen=np.full((M, nbm), -1, np.int32), src=[])
    if cand.shape[1] == 0:
        res["templates"] = [s.copy() for s in sets]
        res["src"] = [np.stack([np.full(len(s), j), np.arange(len(s))], axis=1).astype(np.int32) for j, s in enumerate(sets)]
        return res
    obj = np.arange(M, dtype=np.int32)
    md, so = restate_match(sets, halves, obj, cand, grid)
    offs, chosen, out, src = restate_select(sets, obj, cand, siou, md, so, own, nbm, common["num_extra_coords"], common["iou_thresh"],
                                            params["ex_coords_ratio"], nearest_sq(params["nearest_dist"]))
    res.update(max_dist=md, sel_occ=so, chosen=chosen, templates=[out[offs[g]:offs[g + 1]] for g in range(M)],
               src=[src[offs[g]:offs[g + 1]] for g in range(M)])
    return res


# ------------------------------------------------------------------------------------------------------------------ float64 brute force
def brute_far(target, source, dist):
    """rows of target whose nearest row of source is farther than dist (remove_voxelpnts with nearest_dist), float64"""
    if target.shape[0] == 0:
        return np.zeros((0,), bool)
    if source.shape[0] == 0:
        return np.ones((target.shape[0],), bool)
    d = np.sqrt(((target[:, None, :] - source[None, :, :]) ** 2).sum(-1)).min(axis=1)
    return d > dist


def brute_cells(points, grid):
    ij = np.floor((points[:, :2] - np.array([float(grid["x0"]), float(grid["y0"])])) / float(grid["cell"])).astype(int)
    return {(a, b) for a, b in ij.tolist() if 0 <= a < grid["nx"] and 0 <= b < grid["ny"]}


def brute_class(sets, boxes, params, top_k, iou, common=COMMON, audit=None):
    """steps 3-6 in float64 over the same float32 sets, worded as find_multi_best_match_boxpnts words them: lists that lose the winner.
    -> chosen (M, max_num_bm), per object the list of (source, kept rows).  audit: a list that receives, per round run, (object, the gap
    between the smallest and the second smallest finite h or None)"""
    M = len(sets)
    S = [s.astype(np.float64) for s in sets]
    grid = make_grid(sets, common["cell"])
    cells = [brute_cells(s, grid) for s in S]
    eligible = np.array([len(c) > params["pnt_thresh"] for c in cells])
    cand, siou = top_candidates(iou, eligible, top_k)
    nbm = params["max_num_bm"]
    chosen, segs_all = np.full((M, nbm), -1, np.int32), []
    for i in range(M):
        segs = [(i, np.arange(S[i].shape[0]))]
        dims = np.asarray(boxes[i], np.float64)[3:6]
        ids, ious = list(cand[i]), [float(v) for v in siou[i]]
        picked = [S[c] for c in ids]                  # picked_mirrored_pnts_lst: the one list the reference does not delete the winner from
        picked_ids = list(ids)
        sel = [brute_cells(S[c][np.all((S[c] <= dims * 0.5) & (S[c] >= -dims * 0.5), axis=1)], grid) for c in ids]
        far = []
        for c in ids:
            if S[i].shape[0] == 0:
                far.append(0.0)
            else:
                far.append(float(np.sqrt(((S[i][:, None, :] - S[c][None, :, :]) ** 2).sum(-1)).min(axis=1).max()))
        aug, aug_num = set(cells[i]), 0
        for rnd in range(nbm if ids else 0):
            extra = [len(s - aug) for s in sel]
            h = [far[k] + (params["ex_coords_ratio"] / extra[k] if extra[k] else np.inf) + (ious[k] < common["iou_thresh"]) * 2.0 +
                 (extra[k] < 30) * 1.0 for k in range(len(ids))]
            w = int(np.argmin(h))
            cur = np.concatenate([S[j][r] for j, r in segs], axis=0)
            if audit is not None:
                fin = sorted(v for v in h if np.isfinite(v))
                audit.append((i, fin[1] - fin[0] if len(fin) > 1 else None))
            if (ious[w] < common["iou_thresh"] and cur.shape[0] > 0) or extra[w] == 0:
                break
            keep = np.nonzero(brute_far(picked[w], cur, params["nearest_dist"]))[0]
            if keep.shape[0] > 4:
                segs.append((picked_ids[w], keep))
                chosen[i, rnd] = picked_ids[w]
                aug = aug | sel[w]
                aug_num = len(aug)
            if len(ids) == 1 or aug_num >= common["num_extra_coords"]:
                break
            for lst in (ids, ious, sel, far):
                del lst[w]
        segs_all.append(segs)
    return chosen, segs_all


# ------------------------------------------------------------------------------------------------------------------- the golden file
def load_golden(path, name):
    """tests/golden/templates.npz (gen_templates_golden.py) for one class -> dict(boxes (M, 7) f64, rows: list of (n, 4) f32, image_idx,
    gt_idx, runs: top_k -> dict(templates list, chosen, added, set_counts, cand, iou))"""
    z = np.load(path)
    counts = z[name + "_row_counts"]
    cut = lambda flat, c: [flat[a:a + n] for a, n in zip(np.cumsum(c) - c, c)]
    out = dict(boxes=z[name + "_boxes"], rows=cut(z[name + "_rows"], counts), image_idx=z[name + "_image_idx"], gt_idx=z[name + "_gt_idx"], runs={})
    for key in z.files:
        if key.startswith(name + "_k") and key.endswith("_templates"):
            k = int(key[len(name) + 2:-len("_templates")])
            pre = "%s_k%d_" % (name, k)
            out["runs"][k] = dict(templates=cut(z[pre + "templates"], z[pre + "counts"]), chosen=z[pre + "chosen"], added=z[pre + "added"],
                                  set_counts=z[pre + "set_counts"], cand=z[pre + "cand"], iou=z[pre + "iou"])
    return out


def golden_sets(gold, name):
    """steps 1 and 2 restated over a golden class -> list of (n, 3) float32 sets"""
    kept = [restate_normalize(r, b, COMMON["bottom"]) for r, b in zip(gold["rows"], gold["boxes"])]
    return [restate_mirror(k, COMMON["mirror_dist"]) for k in kept] if CLASS_PARAMS[name]["mirror"] else kept


def ulp_apart(a, b):
    """the largest distance in float32 steps between two float32 arrays of one shape and one sign pattern"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.size == 0:
        return 0
    assert np.array_equal(np.signbit(a), np.signbit(b)) or np.all((a == 0) | (np.signbit(a) == np.signbit(b)))
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


class FakeBank(object):
    """what TemplateBuilder reads of an ObjectBank: table, rows, tensor()"""

    def __init__(self, rows, table):
        self.rows, self.table = rows, table

    def tensor(self, device):
        import torch
        return torch.from_numpy(self.rows).to(device)


class FakeDatabase(object):
    def __init__(self, db_infos, bank):
        self.db_infos, self.bank = db_infos, bank


def golden_databases(golds, split_at=7, box_dtype=np.float64):
    """two databases (objects [0, split_at) and the rest of every class) over the golden classes, as GtDatabase leaves them: db_infos
    with box3d_lidar / image_idx / gt_idx / path, a bank with a table path -> (first_row, n_rows)"""
    dbs = []
    for part in (0, 1):
        infos, parts, table, first = {}, [], {}, 0
        for name, gold in golds.items():
            M = len(gold["rows"])
            for j in (range(0, split_at) if part == 0 else range(split_at, M)):
                path = "gt_database/%06d_%s_%d.bin" % (gold["image_idx"][j], name, j)
                infos.setdefault(name, []).append({"name": name, "path": path, "image_idx": "%06d" % gold["image_idx"][j], "gt_idx": int(gold["gt_idx"][j]),
                                                   "box3d_lidar": gold["boxes"][j].astype(box_dtype)})
                table[path] = (first, gold["rows"][j].shape[0])
                parts.append(gold["rows"][j])
                first += gold["rows"][j].shape[0]
        dbs.append(FakeDatabase(infos, FakeBank(np.ascontiguousarray(np.concatenate(parts, axis=0), F), table)))
    return dbs
