#!/usr/bin/env python3
"""The best-match templates of a KITTI directory, made on the GPU: what the reference's btcdet/datasets/multifindbestfit.py writes.

    python tools/create_templates.py ROOT [--classes Car Cyclist Pedestrian] [--splits train val] [--top-k 800] [--budget-mib 512]

Reads ROOT/kitti_infos_<split>.pkl and ROOT/training/velodyne/*.bin, cuts the ground-truth database of every split on the device
(GtDatabase.build: nothing is read back from ROOT/gt_database*), builds the templates of --classes over the objects of all splits in
the order given (btcdet_amd/template_builder.py: TemplateBuilder.build) and writes
ROOT/bm_<ratio>maxdist_<n>num_<Class>/<image_idx>_<gt_idx>.pkl, a pickled float32 (n, 3) array each.  Prints per class the object
count, the candidates per object, the grid and the size of the bank.  The shipped model configuration names the Cyclist and Pedestrian
directories `..._2num_...`; the reference's script (and so this tool) makes them with max_num_bm 1 and names them `..._1num_...`:
pass --max-num-bm Cyclist=2 Pedestrian=2 for the other."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("root")
    ap.add_argument("--classes", nargs="*", default=["Car", "Cyclist", "Pedestrian"])
    ap.add_argument("--splits", nargs="*", default=["train", "val"])
    ap.add_argument("--top-k", type=int, default=800)
    ap.add_argument("--budget-mib", type=int, default=512, help="device bytes one batch of objects may take")
    ap.add_argument("--max-num-bm", nargs="*", default=[], metavar="CLASS=N")
    ap.add_argument("--frames-per-batch", type=int, default=16)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from btcdet_amd.gt_database import GtDatabase
    from btcdet_amd.kitti_frames import KittiFrames
    from btcdet_amd.template_builder import TemplateBuilder
    dbs = [GtDatabase.build(KittiFrames(args.root, split, fov_points_only=False), used_classes=args.classes, frames_per_batch=args.frames_per_batch,
                            device=args.device) for split in args.splits]
    over = {kv.split("=")[0]: {"max_num_bm": int(kv.split("=")[1])} for kv in args.max_num_bm}
    tb = TemplateBuilder(dbs, top_k=args.top_k, class_params=over, budget_bytes=args.budget_mib << 20, device=args.device)
    t0 = time.perf_counter()
    bank = tb.build(args.classes)
    rows = bank.rows                                   # the one copy down; also the synchronisation the clock needs
    dt = time.perf_counter() - t0
    dirs = tb.save(args.root)
    for name in args.classes:
        print("Templates %s: %s -> %s" % (name, tb.stats[name], dirs[name]))
    print("%d templates, %d rows, %.1f MiB, %.1f s" % (len(bank.table), rows.shape[0], bank.nbytes / 2 ** 20, dt))
    return tb


if __name__ == "__main__":
    main()
