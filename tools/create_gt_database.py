#!/usr/bin/env python3
"""The ground-truth database of a KITTI directory, cut on the GPU: what the reference's `create_groundtruth_database` writes.

    python tools/create_gt_database.py ROOT [--split train] [--classes Car Pedestrian Cyclist] [--frames-per-batch 16]

Reads ROOT/kitti_infos_<split>.pkl (with gt_boxes_lidar in the annos) and ROOT/training/velodyne/*.bin, writes
ROOT/gt_database[_<split>]/*.bin and ROOT/kitti_dbinfos_<split>.pkl (btcdet_amd/gt_database.py: GtDatabase.build + save), and prints
the per-class counts the reference prints.  Every object gets a file; only --classes (default: all) get a db_info.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("root")
    ap.add_argument("--split", default="train")
    ap.add_argument("--classes", nargs="*", default=None, help="used_classes (default: every name in the annos)")
    ap.add_argument("--frames-per-batch", type=int, default=16)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from btcdet_amd.gt_database import GtDatabase
    from btcdet_amd.kitti_frames import KittiFrames
    frames = KittiFrames(args.root, args.split, fov_points_only=False)
    db = GtDatabase.build(frames, used_classes=args.classes or None, frames_per_batch=args.frames_per_batch, device=args.device)
    path = db.save(args.root)
    for name, entries in db.db_infos.items():
        print("Database %s: %d" % (name, len(entries)))
    print("%d objects, %d rows -> %s" % (len(db.objects), int(db.num_points.sum()), path))
    return db


if __name__ == "__main__":
    main()
