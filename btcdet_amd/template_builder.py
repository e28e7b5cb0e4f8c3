"""The best-match templates of `add_multi_best_match`, made on the GPU from the objects of ground-truth databases that already live in
HBM (csrc/template_match.hip, include/btcdet_hip_templates.h).

    train = GtDatabase.build(KittiFrames(root, "train", fov_points_only=False))
    val = GtDatabase.build(KittiFrames(root, "val", fov_points_only=False))
    tb = TemplateBuilder([train, val])
    bank = tb.build(["Car", "Cyclist", "Pedestrian"])          # a TemplateBank whose rows never left the device
    DeviceAugmentor(augmentor, train.bank, templates=bank)
    tb.save(root)                                              # bm_<ratio>maxdist_<n>num_<Class>/<image_idx>_<gt_idx>.pkl

What is replaced: the reference's btcdet/datasets/multifindbestfit.py (its __main__, extract_allpnts, find_best_match_boxpnts), which
needs mayavi, a JIT-compiled CUDA chamfer extension, the compiled iou3d op and its author's paths.  Per class, over the objects of all
databases in the order given (the reference: train, then val):

  1 normalise  the object's rows rotated by -heading about z, rows with z > -dz/2 + bottom kept.  For a float64 box3d_lidar (what the
               KITTI infos carry) on the device: the float32 point promoted, x*c - y*s and x*s + y*c in double from np.cos / np.sin
               formed on the host, one rounding to float32.  An object whose box3d_lidar is NOT float64 takes a host numpy route for this
               stage (normalize_host: the same expressions, whose dtype then follows numpy's promotion) and is uploaded.
  2 mirror     (x, -y, z) of every kept row whose nearest kept row is farther than float32(0.05) is appended (btc_nn_sqdist).
  3 box IoU    boxes_iou3d_gpu of [0, 0, 0, dx, dy, dz, 0] in row blocks, the top `top_k` ELIGIBLE objects per row; an object is eligible
               when its own occupancy count exceeds PNT_THRESH.  Equal IoUs are ordered by lower object index (a stable sort) -- the
               reference leaves that to CUDA topk.  With fewer than top_k eligible objects all of them are candidates (the reference's
               topk raises there).
  4 bitmaps    one grid for the class from the extremes of all sets (btc_match_candidates with the object as its own candidate).
  5, 6         btc_match_candidates and btc_select_templates per batch of G objects; G comes from `budget_bytes` (batch_objects: sel_occ is
               G*K*W*4 bytes; the candidates, the IoU row block, the select workspace and the template rows are counted too).  Per batch only the template offsets are read back.

The greedy bookkeeping (which object is which file) and the file naming stay on the host.  Not here: clustering, t-SNE and every
visualisation of the reference's file, findbestfit.py / finddiff.py, Waymo, ABLATION / filter_bm."""
import os
import pathlib
import pickle

import numpy as np
import torch

from .device_augmentor import TemplateBank

CLASS_PARAMS = {      # the table of the reference's __main__
    "Car": dict(mirror=True, pnt_thresh=80, ex_coords_ratio=50, max_num_bm=2, nearest_dist=0.10),
    "Cyclist": dict(mirror=True, pnt_thresh=5, ex_coords_ratio=5, max_num_bm=1, nearest_dist=0.05),
    "Pedestrian": dict(mirror=False, pnt_thresh=5, ex_coords_ratio=5, max_num_bm=1, nearest_dist=0.05),
}
MAX_NUM_BM_LIMIT = 8


def nearest_sq(nearest_dist):
    """the largest float32 whose correctly rounded square root is <= float32(nearest_dist): d2 > nearest_sq is the reference's
    sqrt(d2) > nearest_dist (a float32 array against a Python float) decision for decision"""
    nd = np.float32(nearest_dist)
    t = np.float32(nd * nd)
    while np.sqrt(t) <= nd:
        t = np.nextafter(t, np.float32(np.inf))
    while np.sqrt(t) > nd:
        t = np.nextafter(t, np.float32(0))
    return t


def normalize_host(rows, box, bottom):
    """step 1 on the host for a box of any dtype -> (n, 3) float32.  c = cos(-heading) and s = sin(-heading) take the box's dtype, and
    x*c - y*s, x*s + y*c and z > -dz/2 + bottom follow numpy's promotion of float32 rows with it: float32 throughout for a float32
    box, double with one rounding for a float64 one.  The reference forms the same two sums with a BLAS matmul, whose order and
    contraction are not defined: for a float32 box its coordinates are within 2 float32 steps of the larger product of these."""
    pts = np.asarray(rows, np.float32)[:, :3]
    c, s = np.cos(-box[6]), np.sin(-box[6])
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.stack([x * c - y * s, x * s + y * c, z], axis=1)
    if bottom != 0.0:
        out = out[z > (-box[5] / 2 + bottom)]
    return out.astype(np.float32)


def directory_name(class_name, params):
    return "bm_{}maxdist_{}num_{}".format(params["ex_coords_ratio"], params["max_num_bm"], class_name)


def file_name(info):
    return str(int(info["image_idx"])) + "_" + str(int(info["gt_idx"])) + ".pkl"


def batch_objects(budget_bytes, K, W, eligible, M, max_num_bm=0, max_rows=0):
    """G, the objects of one batch: what `budget_bytes` holds, per object, of sel_occ (K*W*4), cand + iou + max_dist (K*12), the IoU
    row block with its sorted copy and int64 order (eligible*16), the flag bytes of btc_select_templates' workspace
    (max_num_bm*max_rows) and the template rows at their bound ((1 + max_num_bm)*max_rows*12); at least 1, at most M"""
    per = int(K) * int(W) * 4 + int(K) * 12 + int(eligible) * 16 + int(max_num_bm) * int(max_rows) * (1 + 12) + int(max_rows) * 12
    return int(min(max(int(budget_bytes) // max(per, 1), 1), max(int(M), 1)))


def grid_of(lo, hi, cell):
    """x0, y0 float32 and nx, ny = ceil(extent / cell) in double from the class's float32 extremes (lo, hi: 2 values each, or None)"""
    if lo is None:
        return dict(x0=np.float32(0), y0=np.float32(0), cell=np.float32(cell), nx=1, ny=1)
    nx = max(int(np.ceil((float(hi[0]) - float(lo[0])) / cell)), 1)
    ny = max(int(np.ceil((float(hi[1]) - float(lo[1])) / cell)), 1)
    return dict(x0=np.float32(lo[0]), y0=np.float32(lo[1]), cell=np.float32(cell), nx=nx, ny=ny)


def _popcount_rows(words):
    """(M, W) int32 bit patterns on the device -> (M) int64 set bits"""
    shifts = torch.arange(32, device=words.device, dtype=torch.int32)
    return ((words.unsqueeze(-1) >> shifts) & 1).sum(dim=(1, 2))


class TemplateBuilder(object):
    """databases: GtDatabase objects (their db_infos and bank are used).  Every parameter of the reference's script is a keyword;
    class_params overrides or adds rows of CLASS_PARAMS.  After build(): bank (a TemplateBank), chosen[class] (M, max_num_bm) host
    int32 (object index per round, -1 = nothing added), infos[class], stats[class]."""

    def __init__(self, databases, top_k=800, iou_thresh=0.90, num_extra_coords=2000, cell=0.16, bottom=0.15, mirror_dist=0.05,
                 class_params=None, budget_bytes=512 << 20, device="cuda"):
        self.databases = list(databases)
        self.top_k, self.iou_thresh, self.num_extra_coords = int(top_k), float(iou_thresh), int(num_extra_coords)
        self.cell, self.bottom, self.mirror_dist = float(cell), float(bottom), float(mirror_dist)
        self.class_params = {k: dict(v) for k, v in CLASS_PARAMS.items()}
        for k, v in (class_params or {}).items():
            self.class_params[k] = dict(self.class_params.get(k, {}), **v)
        for k, v in self.class_params.items():
            if not 1 <= int(v["max_num_bm"]) <= MAX_NUM_BM_LIMIT:
                raise ValueError("class %s: max_num_bm %s is outside 1..%d" % (k, v["max_num_bm"], MAX_NUM_BM_LIMIT))
        if self.top_k < 1:
            raise ValueError("top_k must be at least 1")
        self.budget_bytes, self.device = int(budget_bytes), device
        self.bank, self.chosen, self.infos, self.stats, self.built = None, {}, {}, {}, []

    # ------------------------------------------------------------------------------------------------------------------------ host
    def class_objects(self, class_name):
        """-> list of (database index, db_info, first_row, n_rows) in the reference's order: the databases as given, db_infos order"""
        out = []
        for d, db in enumerate(self.databases):
            for info in db.db_infos.get(class_name, []):
                if info["name"] != class_name:
                    continue
                first, n = db.bank.table[info["path"]]
                out.append((d, info, int(first), int(n)))
        return out

    def save(self, root):
        """writes <root>/bm_<ratio>maxdist_<n>num_<Class>/<image_idx>_<gt_idx>.pkl, each a pickled float32 (n, 3) array as the
        reference pickles them: what TemplateBank(template_root) and the reference's MltBestMatchQuerier read.  -> class -> directory"""
        if self.bank is None:
            raise ValueError("TemplateBuilder.save: nothing was built")
        root, rows, dirs = pathlib.Path(root), self.bank.rows, {}
        for name in self.built:
            directory = root / directory_name(name, self.class_params[name])
            os.makedirs(directory, exist_ok=True)
            for info in self.infos[name]:
                first, n = self.bank.table[(name, int(info["image_idx"]), int(info["gt_idx"]))]
                with open(directory / file_name(info), "wb") as f:
                    pickle.dump(np.ascontiguousarray(rows[first:first + n], dtype=np.float32), f)
            dirs[name] = directory
        return dirs

    # ---------------------------------------------------------------------------------------------------------------------- device
    def _upload(self, a, dtype=None):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return (t if dtype is None else t.to(dtype)).to(self.device)

    def normalized_sets(self, objs):
        """step 1 -> (points (N, 3) f32 on the device, object-major; the object of every row (N) int64 on the device; counts (M) host
        int64)"""
        dev, M = self.device, len(objs)
        boxes = [np.asarray(o[1]["box3d_lidar"]) for o in objs]
        on_dev = np.array([b.dtype == np.float64 for b in boxes], dtype=bool)
        parts, oids = [], []
        for d, db in enumerate(self.databases):
            mine = [j for j in range(M) if objs[j][0] == d and on_dev[j] and objs[j][3] > 0]
            if not mine:
                continue
            bank = db.bank.tensor(dev)
            first = self._upload(np.array([objs[j][2] for j in mine], np.int64))
            cnt = self._upload(np.array([objs[j][3] for j in mine], np.int64))
            oid = torch.repeat_interleave(self._upload(np.array(mine, np.int64)), cnt)
            start = torch.cumsum(cnt, 0) - cnt
            idx = torch.repeat_interleave(first - start, cnt) + torch.arange(int(cnt.sum()), device=dev)
            parts.append(bank[idx, :3])
            oids.append(oid)
        kept, kept_oid = torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0,), dtype=torch.int64, device=dev)
        if parts:
            p, oid = torch.cat(parts).double(), torch.cat(oids)
            heading = np.array([float(b[6]) if ok else 0.0 for b, ok in zip(boxes, on_dev)], np.float64)
            thr = np.array([-float(b[5]) / 2 + self.bottom if ok else 0.0 for b, ok in zip(boxes, on_dev)], np.float64)
            c, s, thr = self._upload(np.cos(-heading))[oid], self._upload(np.sin(-heading))[oid], self._upload(thr)[oid]
            x = p[:, 0] * c - p[:, 1] * s
            y = p[:, 0] * s + p[:, 1] * c
            keep = p[:, 2] > thr if self.bottom != 0.0 else torch.ones_like(oid, dtype=torch.bool)
            kept, kept_oid = torch.stack([x, y, p[:, 2]], dim=1)[keep].float(), oid[keep]
        host = [j for j in range(M) if not on_dev[j]]
        if host:
            rows = {d: db.bank.rows for d, db in enumerate(self.databases) if any(objs[j][0] == d for j in host)}
            made = [normalize_host(rows[objs[j][0]][objs[j][2]:objs[j][2] + objs[j][3]], boxes[j], self.bottom) for j in host]
            kept = torch.cat([kept, self._upload(np.concatenate(made, axis=0).reshape(-1, 3))])
            kept_oid = torch.cat([kept_oid, self._upload(np.repeat(np.array(host, np.int64), [m.shape[0] for m in made]))])
        order = torch.sort(kept_oid, stable=True)[1]        # object-major, rows in their order
        kept, kept_oid = kept[order].contiguous(), kept_oid[order]
        return kept, kept_oid, torch.bincount(kept_oid, minlength=M).cpu().numpy().astype(np.int64)

    def nn_sqdist(self, q, t, pairs):
        """btc_nn_sqdist: q, t (., 3) f32 device tensors, pairs (P, 4) host ints -> out (sum q_rows) f32 on the device"""
        from ._lib import check, lib, ptr, stream_ptr
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 4)
        offs = np.concatenate([[0], np.cumsum(pairs[:, 1], dtype=np.int64)])
        if offs[-1] >= 2 ** 31:
            raise ValueError("nn_sqdist: %d query rows do not fit 31 bits" % offs[-1])
        P, total = pairs.shape[0], int(offs[-1])
        out = torch.empty((total,), dtype=torch.float32, device=self.device)
        d_pairs, d_offs = self._upload(pairs), self._upload(offs.astype(np.int32))
        q, t = q.contiguous(), t.contiguous()
        check(lib().btc_nn_sqdist(ptr(q) if q.shape[0] else None, q.shape[0], ptr(t) if t.shape[0] else None, t.shape[0],
                                  ptr(d_pairs) if P else None, ptr(d_offs) if P else None, P, total, ptr(out) if total else None, stream_ptr()),
              "btc_nn_sqdist")
        return out

    def mirrored_sets(self, kept, kept_oid, counts, mirror):
        """step 2 -> (points (N', 3) f32 on the device, seg (M, 2) host int32)"""
        M = counts.shape[0]
        if mirror and kept.shape[0]:
            first = np.cumsum(counts) - counts
            flipped = kept * torch.tensor([1.0, -1.0, 1.0], device=kept.device)
            d2 = self.nn_sqdist(flipped, kept, np.stack([first, counts, first, counts], axis=1))
            far = d2 > float(nearest_sq(self.mirror_dist))
            oid = torch.cat([kept_oid, kept_oid[far]])
            order = torch.sort(oid, stable=True)[1]          # per object: its kept rows, then the mirrored ones, each in order
            kept = torch.cat([kept, flipped[far]])[order].contiguous()
            counts = torch.bincount(oid, minlength=M).cpu().numpy().astype(np.int64)
        if kept.shape[0] >= 2 ** 31:
            raise ValueError("the sets of one class hold %d rows: they are addressed with int32" % kept.shape[0])
        seg = np.stack([np.cumsum(counts) - counts, counts], axis=1).astype(np.int32)
        return kept, seg

    def match(self, points, d_seg, d_half, M, d_obj, d_cand, grid):
        """btc_match_candidates -> max_dist (G, K) f32, sel_occ (G, K, W) i32 bit patterns"""
        from ._lib import check, lib, ptr, stream_ptr
        G, K = d_cand.shape
        W = (grid["nx"] * grid["ny"] + 31) // 32
        md = torch.empty((G, K), dtype=torch.float32, device=self.device)
        so = torch.empty((G, K, W), dtype=torch.int32, device=self.device)
        n = points.shape[0]
        check(lib().btc_match_candidates(ptr(points) if n else None, n, ptr(d_seg) if M else None, ptr(d_half) if M else None, M, ptr(d_obj) if G else None,
                                         ptr(d_cand) if G else None, G, K, float(grid["x0"]), float(grid["y0"]), float(grid["cell"]), grid["nx"],
                                         grid["ny"], ptr(md) if G else None, ptr(so) if G else None, stream_ptr()), "btc_match_candidates")
        return md, so

    def select(self, points, d_seg, M, d_obj, d_cand, d_iou, md, so, own, params, max_rows, capacity, want_src=False):
        """btc_select_templates, called again when the templates outgrow `capacity` -> out (total, 3), offsets host int64 (G+1), chosen
        (G, max_num_bm) device i32 [, src (total, 2) device i32]"""
        from ._lib import check, lib, ptr, stream_ptr, workspace
        L = lib()
        G, K = d_cand.shape
        W, nbm, n = so.shape[2], int(params["max_num_bm"]), points.shape[0]
        offs = torch.empty((G + 1,), dtype=torch.int32, device=self.device)
        chosen = torch.empty((G, nbm), dtype=torch.int32, device=self.device)
        ws_bytes = L.btc_select_templates_ws_bytes(G, nbm, max_rows)
        ws = workspace(ws_bytes, self.device)

        def call(cap):
            out = torch.empty((cap, 3), dtype=torch.float32, device=self.device)
            src = torch.empty((cap, 2), dtype=torch.int32, device=self.device) if want_src else None
            check(L.btc_select_templates(ptr(points) if n else None, n, ptr(d_seg) if M else None, M, ptr(d_obj) if G else None, ptr(d_cand) if G else None,
                                         ptr(d_iou) if G else None, ptr(md) if G else None, ptr(so) if G else None, ptr(own) if M else None, G, K, W, nbm,
                                         self.num_extra_coords, self.iou_thresh, float(params["ex_coords_ratio"]),
                                         float(nearest_sq(params["nearest_dist"])), max_rows, cap, ptr(out) if cap else None,
                                         ptr(src) if (want_src and cap) else None, ptr(offs), ptr(chosen), ptr(ws), ws_bytes, stream_ptr()),
                  "btc_select_templates")
            return out, src, offs.cpu().numpy().astype(np.int64)

        out, src, bounds = call(int(capacity))
        if bounds[-1] > capacity:
            out, src, bounds = call(int(bounds[-1]))
        total = int(bounds[-1])
        return (out[:total], bounds, chosen, src[:total]) if want_src else (out[:total], bounds, chosen)

    def build_class(self, class_name, iou_fn=None):
        """the templates of one class -> (rows (total, 3) f32 on the device, offsets host int64 (M+1), infos).  iou_fn(boxes_a, boxes_b)
        -> (a, b) float32 on the device stands in for iou3d_nms.boxes_iou3d_gpu: the tests feed equal IoUs through it."""
        if class_name not in self.class_params:
            raise KeyError("no parameters for class %r: pass class_params" % class_name)
        if iou_fn is None:
            from .iou3d_nms import boxes_iou3d_gpu as iou_fn
        params, dev = self.class_params[class_name], self.device
        objs = self.class_objects(class_name)
        M = len(objs)
        infos = [o[1] for o in objs]
        self.infos[class_name] = infos
        nbm = int(params["max_num_bm"])
        if M == 0:
            self.chosen[class_name] = np.zeros((0, nbm), np.int32)
            self.stats[class_name] = dict(objects=0)
            return torch.zeros((0, 3), dtype=torch.float32, device=dev), np.zeros((1,), np.int64), infos
        kept, kept_oid, counts = self.normalized_sets(objs)
        points, seg = self.mirrored_sets(kept, kept_oid, counts, bool(params["mirror"]))
        n, max_rows = points.shape[0], int(seg[:, 1].max())
        lo = hi = None
        if n:
            lo, hi = points[:, :2].amin(dim=0).cpu().numpy(), points[:, :2].amax(dim=0).cpu().numpy()
        grid = grid_of(lo, hi, self.cell)
        dims = np.stack([np.asarray(i["box3d_lidar"], np.float64)[3:6] for i in infos])
        d_seg, d_half = self._upload(seg), self._upload((dims / 2).astype(np.float32))
        every = torch.arange(M, dtype=torch.int32, device=dev)
        _, own = self.match(points, d_seg, torch.full((M, 3), float("inf"), device=dev), M, every, every.view(M, 1).contiguous(), grid)
        own = own.view(M, -1).contiguous()
        eligible = torch.nonzero(_popcount_rows(own) > int(params["pnt_thresh"]))[:, 0]
        E = int(eligible.shape[0])
        K, W = min(self.top_k, E), own.shape[1]
        self.stats[class_name] = dict(objects=M, rows=n, eligible=E, K=K, nx=grid["nx"], ny=grid["ny"], W=W, max_rows=max_rows)
        if K == 0:                                                   # nothing to match against: every template is the object's own set
            self.chosen[class_name] = np.full((M, nbm), -1, np.int32)
            return points, np.concatenate([[0], np.cumsum(seg[:, 1], dtype=np.int64)]), infos
        boxes = torch.zeros((M, 7), dtype=torch.float32, device=dev)
        boxes[:, 3:6] = self._upload(dims, torch.float32)
        G = batch_objects(self.budget_bytes, K, W, E, M, nbm, max_rows)
        self.stats[class_name]["G"] = G
        pieces, chosen, bounds = [], [], [0]
        for a in range(0, M, G):
            b = min(a + G, M)
            iou = iou_fn(boxes[a:b], boxes[eligible])
            siou, order = torch.sort(iou, dim=1, descending=True, stable=True)
            d_iou = siou[:, :K].contiguous()
            d_cand = eligible[order[:, :K]].to(torch.int32).contiguous()
            d_obj = every[a:b].contiguous()
            md, so = self.match(points, d_seg, d_half, M, d_obj, d_cand, grid)
            own_rows = int(seg[a:b, 1].sum())
            out, offs, ch = self.select(points, d_seg, M, d_obj, d_cand, d_iou, md, so, own, params, max_rows, own_rows * 2 + 64)
            pieces.append(out)
            chosen.append(ch)
            bounds.extend((offs[1:] + bounds[-1]).tolist())
        self.chosen[class_name] = torch.cat(chosen).cpu().numpy()
        return torch.cat(pieces), np.array(bounds, np.int64), infos

    def build(self, classes, iou_fn=None):
        """-> a TemplateBank over rows that never left the device; table (class, image_idx, gt_idx) -> (first_row, n_rows)"""
        table, pieces, first = {}, [], 0
        self.built = []
        for name in classes:
            rows, bounds, infos = self.build_class(name, iou_fn)
            for j, info in enumerate(infos):
                table[(str(name), int(info["image_idx"]), int(info["gt_idx"]))] = (first + int(bounds[j]), int(bounds[j + 1] - bounds[j]))
            pieces.append(rows)
            first += int(bounds[-1])
            self.built.append(name)
        if first >= 2 ** 31:
            raise ValueError("TemplateBuilder.build: %d template rows do not fit 31 bits" % first)
        rows = torch.cat(pieces) if pieces else torch.zeros((0, 3), dtype=torch.float32, device=self.device)
        self.bank = TemplateBank.from_rows(None, table, device_rows=rows)
        return self.bank
