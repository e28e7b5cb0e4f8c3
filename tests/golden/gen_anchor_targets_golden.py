"""Golden vectors of the anchor head's target assignment and box decoding, produced by the reference's OWN modules run here on the CPU
(through ref_env): AxisAlignedTargetAssigner.assign_targets with the ResidualCoder and the anchors AnchorHeadTemplate.generate_anchors
builds, and AnchorHeadTemplate.generate_predicted_boxes.  Inputs and outputs of every case are recorded; the configurations live in
tests/anchor_targets_ref.py (MAPS, head_cfg), which the tests share.

Every input that is not MEANT to sit on an edge passes anchor_targets_ref.margins_assign / margins_decode: 1e-5 around both thresholds,
1e-3 rad around the heading snap, 1e-4 around an integer quotient of the direction bins, no tied logits, no real box summing to zero.
With those margins either form of val / period and any summation order decide alike, so the CPU reference pins what the device computes.

    python tests/golden/gen_anchor_targets_golden.py   ->  tests/golden/anchor_targets.npz"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_env  # noqa: E402
import oracle_spconv  # noqa: E402

ref_env.install(oracle_spconv)
import torch  # noqa: E402

import anchor_targets_ref as ar  # noqa: E402
from btcdet.models.dense_heads.anchor_head_template import AnchorHeadTemplate  # noqa: E402
from btcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner import AxisAlignedTargetAssigner  # noqa: E402
from btcdet.utils import box_coder_utils, box_utils  # noqa: E402

F = np.float32


def ref_anchors(map_name, cfg):
    m = ar.MAPS[map_name]
    gen = [ref_env.EasyDict(g) for g in cfg.ANCHOR_GENERATOR_CONFIG]
    anchors, _ = AnchorHeadTemplate.generate_anchors(gen, grid_size=np.array(m["grid_size"]), point_cloud_range=np.array(m["point_cloud_range"], F),
                                                     anchor_ndim=7)
    return anchors


def ref_assign(map_name, gt, matched=None, unmatched=None):
    cfg = ref_env.EasyDict(ar.head_cfg(map_name, matched, unmatched))
    anchors = ref_anchors(map_name, cfg)
    assigner = AxisAlignedTargetAssigner(cfg, ar.MAPS[map_name]["class_names"], box_coder_utils.ResidualCoder(), match_height=False)
    out = assigner.assign_targets(anchors, torch.from_numpy(gt.copy()))
    flat = torch.cat(anchors, dim=-3).view(-1, 7).numpy()
    return flat, out["box_cls_labels"].numpy(), out["box_reg_targets"].numpy(), out["reg_weights"].numpy(), cfg


def ref_decode(map_name, preds, dirs):
    cfg = ref_env.EasyDict(ar.head_cfg(map_name))
    me = types.SimpleNamespace(anchors=ref_anchors(map_name, cfg), use_multihead=False, box_coder=box_coder_utils.ResidualCoder(), model_cfg=cfg)
    _, boxes = AnchorHeadTemplate.generate_predicted_boxes(me, preds.shape[0], torch.zeros(preds.shape[0], preds.shape[1], 1), torch.from_numpy(preds.copy()),
                                                           None if dirs is None else torch.from_numpy(dirs.copy()))
    return boxes.numpy()


def box(x, y, z, dx, dy, dz, r, c):
    return [x, y, z, dx, dy, dz, r, c]


def padded(rows, M):
    out = np.zeros((M, 8), F)
    if len(rows):
        out[:len(rows)] = np.array(rows, F)
    return out


def assign_cases():
    cases = []
    # ---- the `one` map: anchors (4.0, 1.5) at even x and odd y, every quantity exact in float32
    s0 = [box(5.0, 1.0, -1.0, 3.5, 1.5, 1.5, 0.0, 1),          # centred exactly between the anchors at x = 4 and x = 6: both tie, both are forced
          box(12.0, -5.0, -1.0, 4.0, 1.5, 1.5, 0.0, 1),        # two boxes of one footprint (their z differs, so the targets show which won):
          box(12.0, -5.0, -0.75, 4.0, 1.5, 1.5, 0.0, 1),       # the first index wins
          box(100.0, 100.0, -1.0, 3.9, 1.6, 1.5, 0.3, 1),      # no anchor touches it: forces nothing
          box(20.3, 7.4, -1.2, 1.2, 0.8, 1.4, 0.2, 1),         # small: its best anchors stay below `unmatched` and are forced all the same
          box(8.5, -9.3, -0.9, 3.8, 1.6, 1.5, 1.2, 1)]
    s2 = [box(25.1, 11.2, -1.1, 4.1, 1.7, 1.6, -2.9, 1)]
    cases.append(dict(name="one_mixed", map="one", gt=np.stack([padded(s0, 9), padded([], 9), padded(s2, 9)])))    # 6 / only padding / 1 + 8 pad rows
    cases.append(dict(name="one_row0_padding", map="one", gt=np.stack([padded([[0] * 8, box(14.2, 2.9, -1.0, 3.9, 1.6, 1.5, 0.1, 1)], 4)])))
    cases.append(dict(name="one_five", map="one", gt=ar.random_boxes(np.random.default_rng(5), 5, 1, (1, -14, 29, 14), pad=1)[None]))
    cases.append(dict(name="one_no_rows", map="one", gt=np.zeros((2, 0, 8), F)))                                  # M == 0
    # thresholds ON overlaps: the second largest overlap of the box as `matched` (that anchor is positive by >=), the third as
    # `unmatched` (that anchor is not background by <)
    gt = np.stack([padded([box(10.6, 3.3, -1.0, 3.9, 1.6, 1.5, 0.1, 1)], 2)])
    flat = ref_assign("one", gt)[0]
    iou = box_utils.boxes3d_nearest_bev_iou(torch.from_numpy(flat), torch.from_numpy(gt[0, :1, :7])).numpy()[:, 0]
    vals = np.unique(iou)[::-1]
    assert vals[2] > 0.05 and vals[0] < 1
    cases.append(dict(name="one_on_thresholds", map="one", gt=gt, matched=[float(vals[1])], unmatched=[float(vals[2])],
                      on_edge=int((iou == vals[1]).sum() + (iou == vals[2]).sum()), probe=(iou, vals)))
    # ---- the `three` map: Car / Pedestrian / Cyclist; class 4 (Van) has no configuration, class 0 wraps to it
    t0 = [box(9.7, -3.2, -1.0, 3.7, 1.6, 1.5, 0.3, 1), box(15.3, 6.1, -0.6, 0.7, 0.65, 1.7, 1.9, 2), box(21.2, -8.4, -0.7, 1.8, 0.6, 1.7, -0.4, 3),
          box(12.5, 2.2, -0.8, 5.2, 2.0, 2.1, 0.05, 4), box(4.4, 9.9, -0.6, 0.9, 0.55, 1.8, -1.2, 2)]
    t2 = [box(27.6, 1.3, -0.7, 1.7, 0.62, 1.7, 2.6, 3)]
    cases.append(dict(name="three_mixed", map="three", gt=np.stack([padded(t0, 7), padded([], 7), padded(t2, 7)])))
    for n, seed in ((63, 0), (64, 0), (65, 0)):
        cases.append(dict(name="three_%d" % n, map="three", gt=None, n=n, seed=seed))
    return cases


def seeded_scene(n, seed):
    return ar.random_boxes(np.random.default_rng(1000 * n + seed), n, 4, (1, -13, 31, 13), pad=2)[None]


if __name__ == "__main__":
    gold, index = {}, []
    for c in assign_cases():
        name, mp, matched, unmatched, on_edge = c["name"], c["map"], c.get("matched"), c.get("unmatched"), c.get("on_edge", 0)
        tables = ar.host_tables(ar.head_cfg(mp, matched, unmatched), ar.MAPS[mp]["class_names"])
        gt = c["gt"]
        if gt is None:                                  # seeded scenes: the first seed whose boxes pass the margins
            flat0 = ref_assign(mp, np.zeros((1, 1, 8), F))[0]
            for seed in range(c["seed"], c["seed"] + 50):
                gt = seeded_scene(c["n"], seed)
                try:
                    ar.margins_assign(flat0, *tables, gt)
                    break
                except AssertionError as e:
                    print(name, "seed", seed, "refused:", e)
            else:
                raise SystemExit("no seed passes the margins")
        flat, labels, targets, weights, cfg = ref_assign(mp, gt, matched, unmatched)
        r_lab, r_tgt, r_w, r_best, r_iou, r_forced = ar.margins_assign(flat, *tables, gt, on_edge=on_edge)
        # the restatement against the reference, here where both run
        assert np.array_equal(r_lab, labels) and np.array_equal(r_w, weights), name
        assert np.array_equal(r_tgt[..., list(ar.EXACT)], targets[..., list(ar.EXACT)]), name
        np.testing.assert_allclose(r_tgt, targets, rtol=1e-5, atol=1e-6)
        mine = tables[0][np.arange(flat.shape[0]) % len(tables[0])]
        if name == "one_mixed":
            top0 = r_iou[0][(r_best[0] == 0)].max()
            assert int(((r_best[0] == 0) & (r_iou[0] == top0) & r_forced[0]).sum()) == 2, "two anchors tie the first box"
            assert np.all(r_best[0] != 2) and np.any(r_best[0] == 1), "the first of two identical boxes wins"
            assert np.all(r_best[0] != 3) or np.all(r_iou[0][r_best[0] == 3] == 0), "nothing touches the far box"
            assert np.any((labels[0] > 0) & (r_iou[0] < tables[2][mine])), "an anchor forced below `unmatched`"
            assert np.all(labels[1] == 0) and np.all(weights[1] == 0), "a scene of padding is all background"
        if name == "one_on_thresholds":
            iou, vals = c["probe"]
            assert np.all(labels[0][iou == vals[1]] == 1) and np.all(labels[0][iou == vals[2]] == -1) and np.all(labels[0][iou == vals[0]] == 1)
            assert np.array_equal(r_iou[0], iou)
        if name == "three_mixed":
            assert set(np.unique(labels[0])) == {-1, 0, 1, 2, 3} or set(np.unique(labels[0])) == {0, 1, 2, 3}, np.unique(labels[0])
            assert np.all(r_best[0] != 3), "a class without a configuration is offered to nobody"
        print("%-18s B %d M %2d A %4d  positives %4d  ignored %3d  forced %3d  on a threshold %d" %
              (name, gt.shape[0], gt.shape[1], flat.shape[0], int((labels > 0).sum()), int((labels < 0).sum()), int(r_forced.sum()), on_edge))
        gold["anchors/" + mp] = flat
        gold[name + "/gt"], gold[name + "/labels"], gold[name + "/targets"], gold[name + "/weights"] = gt, labels.astype(np.int8), targets, weights
        index.append(dict(name=name, kind="assign", map=mp, matched=matched, unmatched=unmatched, on_edge=on_edge))
    for name, mp, B, with_dir in (("decode_one", "one", 2, True), ("decode_three", "three", 1, True), ("decode_no_dir", "one", 1, False)):
        cfg = ar.head_cfg(mp)
        flat = gold["anchors/" + mp]
        rng = np.random.default_rng(len(name))
        preds = (rng.standard_normal((B, flat.shape[0], 7)) * 0.4).astype(F)
        dirs = rng.standard_normal((B, flat.shape[0], cfg.NUM_DIR_BINS)).astype(F) if with_dir else None
        if with_dir:                                    # move the few rotations whose quotient lies near an integer
            q = (preds[..., 6].astype(np.float64) + flat[None, :, 6] - cfg.DIR_OFFSET) / (2 * np.pi / cfg.NUM_DIR_BINS) + cfg.DIR_LIMIT_OFFSET
            preds[..., 6] += np.where(np.abs(q - np.round(q)) < 1e-3, F(0.01), F(0))
        ar.margins_decode(preds, flat, dirs, cfg.DIR_OFFSET, cfg.DIR_LIMIT_OFFSET, cfg.NUM_DIR_BINS)
        boxes = ref_decode(mp, preds, dirs)
        for recip in (True, False):
            r = ar.restate_decode(preds, flat, dirs, cfg.DIR_OFFSET, cfg.DIR_LIMIT_OFFSET, cfg.NUM_DIR_BINS, recip)
            assert np.array_equal(r[..., list(ar.EXACT)], boxes[..., list(ar.EXACT)]), name
            np.testing.assert_allclose(r, boxes, rtol=1e-5, atol=1e-6)
        print("%-18s B %d A %4d  dir %s" % (name, B, flat.shape[0], with_dir))
        gold[name + "/box_preds"], gold[name + "/boxes"] = preds, boxes
        if with_dir:
            gold[name + "/dir_cls_preds"] = dirs
        index.append(dict(name=name, kind="decode", map=mp, dir=with_dir))
    gold["cases"] = np.array(json.dumps(index))
    path = os.path.join(HERE, "anchor_targets.npz")
    np.savez_compressed(path, **gold)
    print("wrote anchor_targets.npz %.0f KB" % (os.path.getsize(path) / 1024))
