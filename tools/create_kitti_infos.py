#!/usr/bin/env python3
"""The info pickles of a raw KITTI directory, with the point work on the GPU: what the reference's `create_kitti_infos` and
`create_kitti_infos_with_coverage` write.

    python tools/create_kitti_infos.py ROOT [--save-path DIR] [--frames-per-batch 16]
    python tools/create_kitti_infos.py ROOT --coverage --templates Car=DIR Pedestrian=DIR Cyclist=DIR

Without --coverage: reads ROOT/ImageSets/{train,val,test}.txt, ROOT/training/{velodyne,calib,label_2,image_2} and ROOT/testing/...,
writes kitti_infos_{train,val,test}.pkl, gt_database[_val]/*.bin and kitti_dbinfos_{train,val}.pkl (btcdet_amd/kitti_infos.py:
create_kitti_infos).  With --coverage: reads kitti_infos_{train,val}.pkl and the best-match templates (<image_idx>_<gt_idx>.pkl per
class directory, as tools/create_templates.py or the reference writes them) and writes kitti_cvrg_infos_{train,val}.pkl.
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
    ap.add_argument("--save-path", default=None, help="where the pickles go (default: ROOT)")
    ap.add_argument("--coverage", action="store_true", help="add coverage_rates to the infos that exist")
    ap.add_argument("--templates", nargs="*", default=[], metavar="CLASS=DIR", help="template directories, for --coverage")
    ap.add_argument("--frames-per-batch", type=int, default=16)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from btcdet_amd import kitti_infos
    if args.coverage:
        roots = dict(t.split("=", 1) for t in args.templates)
        if not roots:
            ap.error("--coverage needs --templates CLASS=DIR ...")
        paths = kitti_infos.create_kitti_infos_with_coverage(args.root, roots, args.save_path, frames_per_batch=args.frames_per_batch, device=args.device)
    else:
        paths = kitti_infos.create_kitti_infos(args.root, args.save_path, frames_per_batch=args.frames_per_batch, device=args.device)
    for split, path in paths.items():
        print("%s -> %s" % (split, path))
    return paths


if __name__ == "__main__":
    main()
