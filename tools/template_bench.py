#!/usr/bin/env python3
"""The best-match templates: the reference's own formulation in torch on the GPU against TemplateBuilder.build, alternating in ONE
process.

A synthetic class: --objects objects of 100 - 1500 rows near the surface of boxes whose sides vary by a few percent (so that most box
IoUs are above 0.90, as among KITTI cars), seen from one side, resident as a GtDatabase leaves them.  Car parameters, top_k 800.

  ours      TemplateBuilder.build(["Car"]) over the whole class: objects per second, host clock around the build ending in a device
            synchronisation;
  baseline  multifindbestfit.py's formulation for --base-objects objects of the same class, with the sets, grid, own bitmaps and
            candidates that `ours` made (they are not timed): per object the candidates padded to one tensor and torch.cdist + min
            in chunks (its padded chamfer), the bitmap of every candidate's in-box rows (its remove_outofbox + space_occ_voxelpnts
            stack, vectorised here: kinder than its Python loop), then its Python greedy loop with torch reductions and a cdist filter;
  kernels   btc_nn_sqdist, btc_match_candidates and btc_select_templates alone, between device events, inside the builds of `ours`
            (the select figure includes the read-back of the offsets that ends every batch).

`baseline` is THE BASELINE, not code under test.  Blocks alternate --alternations times.  Writes profiles/template_bench.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=2000)
    ap.add_argument("--base-objects", type=int, default=32, help="objects per baseline block")
    ap.add_argument("--top-k", type=int, default=800)
    ap.add_argument("--alternations", type=int, default=5, help="timed blocks PER PATH (at least 5 for a result that is reported)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "template_bench.json"))
    return ap.parse_args(argv)


class Database(object):
    def __init__(self, db_infos, bank):
        self.db_infos, self.bank = db_infos, bank


def make_class(args, device, seed=21):
    import numpy as np
    import torch
    from btcdet_amd.device_augmentor import ObjectBank
    rng = np.random.default_rng(seed)
    infos, parts, table, first = [], [], {}, 0
    for j in range(args.objects):
        box = np.zeros(7)
        box[3:6] = np.array([3.9, 1.6, 1.56]) * (1 + rng.uniform(-0.03, 0.03, 3))
        box[6] = rng.uniform(-np.pi, np.pi)
        n = int(rng.integers(100, 1501))
        u = rng.normal(size=(3 * n, 3))
        u /= np.abs(u).max(axis=1, keepdims=True)
        local = u * box[3:6] / 2 * rng.uniform(0.9, 1.02, (3 * n, 1))
        view = rng.uniform(0, 2 * np.pi)
        local = local[(local[:, 0] * np.cos(view) + local[:, 1] * np.sin(view)) > -0.3][:n]
        c, s = np.cos(box[6]), np.sin(box[6])
        rows = np.stack([local[:, 0] * c - local[:, 1] * s, local[:, 0] * s + local[:, 1] * c, local[:, 2], rng.uniform(0, 1, local.shape[0])], axis=1)
        path = "gt_database/%06d_Car_0.bin" % j
        infos.append({"name": "Car", "path": path, "image_idx": "%06d" % j, "gt_idx": 0, "box3d_lidar": box})
        table[path] = (first, rows.shape[0])
        parts.append(rows.astype(np.float32))
        first += rows.shape[0]
    bank = ObjectBank.from_rows(None, table, 4, device_rows=torch.from_numpy(np.concatenate(parts)).to(device))
    return Database({"Car": infos}, bank), first


def baseline_objects(state, ids, params, tb):
    """the reference's formulation for the objects `ids` -> template rows made"""
    import torch
    pts, seg, half, grid, own, cand, iou = state["points"], state["seg"], state["half"], state["grid"], state["own"], state["cand"], state["iou"]
    nx, ny, dev = grid["nx"], grid["ny"], pts.device
    x0y0 = torch.tensor([float(grid["x0"]), float(grid["y0"])], device=dev)
    made = 0
    for i in ids:
        ci = cand[i].tolist()
        sets = [pts[seg[c][0]:seg[c][0] + seg[c][1]] for c in ci]
        q = pts[seg[i][0]:seg[i][0] + seg[i][1]]
        lens = torch.tensor([s.shape[0] for s in sets], device=dev)
        padded = torch.nn.utils.rnn.pad_sequence(sets, batch_first=True, padding_value=10.0)           # its reversemask: pads far away
        valid = torch.arange(padded.shape[1], device=dev)[None, :] < lens[:, None]
        far = []
        for a in range(0, len(ci), 64):                                                                  # its padded one-sided chamfer maximum
            d = torch.cdist(q[None].expand(min(64, len(ci) - a), -1, -1), padded[a:a + 64])
            far.append(d.min(dim=2)[0].max(dim=1)[0] if q.shape[0] else torch.zeros(d.shape[0], device=dev))
        max_instance = torch.cat(far)
        inbox = ((padded.abs() <= half[i][None, None, :]).all(dim=2)) & valid                           # remove_outofbox + space_occ_voxelpnts, stacked
        ij = torch.floor((padded[:, :, :2] - x0y0) / 0.16).long()
        ok = inbox & (ij[:, :, 0] >= 0) & (ij[:, :, 0] < nx) & (ij[:, :, 1] >= 0) & (ij[:, :, 1] < ny)
        occ = torch.zeros((len(ci), nx * ny + 1), dtype=torch.int32, device=dev)
        occ.scatter_(1, torch.where(ok, ij[:, :, 0] * ny + ij[:, :, 1], torch.full_like(ij[:, :, 0], nx * ny)), 1)
        selected_occ_map = occ[:, :nx * ny]
        aug_map, sorted_iou, bm_pnts, aug_coords_num = own[i], iou[i], q, 0
        for rnd in range(params["max_num_bm"]):                                                          # find_multi_best_match_boxpnts
            extra = (selected_occ_map * (1 - aug_map)[None, :]).sum(dim=1)
            heuristic = max_instance + params["ex_coords_ratio"] / extra + (sorted_iou < tb.iou_thresh) * 2.0 + (extra < 30) * 1.0
            ind = int(torch.min(heuristic, dim=0)[1].cpu())
            if (float(sorted_iou[ind].cpu()) < tb.iou_thresh and bm_pnts.shape[0] > 0) or int(extra[ind].cpu()) == 0:
                break
            target = sets[ind]
            keep = torch.cdist(target[None], bm_pnts[None])[0].min(dim=1)[0] > params["nearest_dist"] if bm_pnts.shape[0] else torch.ones(target.shape[0], dtype=torch.bool, device=dev)
            added = target[keep]
            if added.shape[0] > 4:
                bm_pnts = torch.cat([bm_pnts, added])
                aug_map = aug_map | selected_occ_map[ind]
                aug_coords_num = int(aug_map.sum().cpu())
            if sorted_iou.shape[0] == 1 or aug_coords_num >= tb.num_extra_coords:
                break
            rest = torch.arange(sorted_iou.shape[0], device=dev) != ind
            sorted_iou, selected_occ_map, max_instance = sorted_iou[rest], selected_occ_map[rest], max_instance[rest]
        made += bm_pnts.cpu().numpy().shape[0]                                                           # it pickles every template
    return made


def measure(args, device):
    import numpy as np
    import torch
    from btcdet_amd import template_builder as B
    events = {"btc_nn_sqdist": [], "btc_match_candidates": [], "btc_select_templates": []}
    state = {}

    class Timed(B.TemplateBuilder):
        def _timed(self, name, fn, *a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            events[name].append((e0, e1))
            return out

        def nn_sqdist(self, *a, **k):
            return self._timed("btc_nn_sqdist", B.TemplateBuilder.nn_sqdist, self, *a, **k)

        def match(self, points, d_seg, d_half, M, d_obj, d_cand, grid):
            out = self._timed("btc_match_candidates", B.TemplateBuilder.match, self, points, d_seg, d_half, M, d_obj, d_cand, grid)
            if d_cand.shape[1] == 1:
                state.update(points=points, seg=d_seg.cpu().tolist(), grid=grid, own_words=out[1].view(M, -1))
            else:
                state.update(half=d_half, cand=d_cand, obj=d_obj)
            return out

        def select(self, points, d_seg, M, d_obj, d_cand, d_iou, *a, **k):
            state.update(iou=d_iou)
            return self._timed("btc_select_templates", B.TemplateBuilder.select, self, points, d_seg, M, d_obj, d_cand, d_iou, *a, **k)

    t0 = time.perf_counter()
    db, n_rows = make_class(args, device)
    setup = time.perf_counter() - t0
    tb = Timed([db], top_k=args.top_k, device=device)
    params = tb.class_params["Car"]

    def ours():
        t0 = time.perf_counter()
        bank = tb.build(["Car"])
        torch.cuda.synchronize()
        return time.perf_counter() - t0, bank

    _, bank = ours()                                       # warm-up; leaves `state` for the baseline
    assert tb.stats["Car"]["G"] >= args.objects, "the baseline reads the candidates of ONE batch: raise the budget"
    nx, ny = state["grid"]["nx"], state["grid"]["ny"]
    shifts = torch.arange(32, device=device, dtype=torch.int32)
    state["own"] = ((state["own_words"].unsqueeze(-1) >> shifts) & 1).reshape(args.objects, -1)[:, :nx * ny].to(torch.int32)
    rng = np.random.default_rng(3)
    baseline_objects(state, rng.choice(args.objects, 2, replace=False).tolist(), params, tb)
    torch.cuda.synchronize()
    for v in events.values():
        del v[:]
    res = {"objects": args.objects, "object_rows": n_rows, "top_k": args.top_k, "stats": {k: int(v) for k, v in tb.stats["Car"].items()},
           "template_rows": int(bank.tensor(device).shape[0]), "bank_bytes": bank.nbytes, "setup_s": round(setup, 2), "base_objects": args.base_objects,
           "objects_per_s": {"baseline": [], "ours": []}}
    for a in range(args.alternations):
        ids = rng.choice(args.objects, args.base_objects, replace=False).tolist()
        t0 = time.perf_counter()
        baseline_objects(state, ids, params, tb)
        torch.cuda.synchronize()
        res["objects_per_s"]["baseline"].append(args.base_objects / (time.perf_counter() - t0))
        dt, _ = ours()
        res["objects_per_s"]["ours"].append(args.objects / dt)
    torch.cuda.synchronize()
    per = {k: len(v) // args.alternations for k, v in events.items()}           # the calls of one build are consecutive
    res["kernel_calls_per_build"] = per
    res["kernel_ms_per_build"] = {k: [round(sum(e0.elapsed_time(e1) for e0, e1 in v[b * per[k]:(b + 1) * per[k]]), 3) for b in range(args.alternations)]
                                  for k, v in events.items()}
    med = {k: statistics.median(v) for k, v in res["objects_per_s"].items()}
    base = res["objects_per_s"]["baseline"]
    res["median_objects_per_s"] = med
    res["baseline_spread"] = (max(base) - min(base)) / med["baseline"]
    res["speedup"] = med["ours"] / med["baseline"]
    return res


def main(argv=None):
    args = parse_args(argv)
    import torch
    import infer_bench
    out = {"head": infer_bench.head_commit(), "alternations": args.alternations, "templates": measure(args, torch.device("cuda:0"))}
    print(json.dumps(out["templates"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
