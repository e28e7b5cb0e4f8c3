"""Golden vectors of the reference's training augmentation (runs only where the reference is mounted): its OWN DataAugmentor.forward
(btcdet/datasets/augmentor/data_augmentor.py:171-202) with its own DataBaseSampler and augmentor_utils, over the small synthetic
database of common.make_gt_database and the three consecutive scenes of tests/augment_cases.py, global numpy RNG seeded with 99, for
the four variants there (both shipped queue orders x REMOVE_EXTRA_WIDTH 0 / 0.2).  The DataAugmentor is made with object.__new__ and its
queue set by hand (its constructor wants database pickles).  The two compiled primitives the sampler calls -- absent here -- are
served by the restatements of gen_sampler_golden.py.

Every output key of every scene is recorded.  The point arrays (points, pre_rot_points, the special sets) are held in full for the
variant augment_cases.FULL and as shape + SHA-1 of their bytes for the other three: twelve full scenes would pass the size limit of a
committed file, and a digest of the bytes still pins them bit for bit.

    python tests/golden/gen_augment_golden.py   ->  tests/golden/augment.npz"""
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gen_sampler_golden as gs  # noqa: E402  (installs the stubs and the two restated primitives, imports the reference's sampler)
import augment_cases as ac  # noqa: E402
import common  # noqa: E402
from btcdet.datasets.augmentor.data_augmentor import DataAugmentor  # noqa: E402

if __name__ == "__main__":
    gold = {}
    for variant in ac.VARIANTS:
        with tempfile.TemporaryDirectory() as d:
            infos = common.make_gt_database(d)
            aug = object.__new__(DataAugmentor)
            aug.data_augmentor_queue = []
            for cfg in ac.queue_cfgs(variant):
                if cfg.NAME == "gt_sampling":
                    aug.data_augmentor_queue.append(gs.DataBaseSampler(Path(d), cfg, ac.CLASSES, infos))
                else:
                    aug.data_augmentor_queue.append(getattr(aug, cfg.NAME)(config=cfg))
            np.random.seed(ac.SEED)
            for i, sc in enumerate(ac.scenes()):
                r = aug.forward(sc)
                ac.record(gold, "%s%d_" % (variant, i), r, full=variant == ac.FULL)
                print(variant, i, r["points"].shape, r["gt_boxes"].shape, r.get("augment_box_num"), r.get("rot_z"), sorted(r))
            gold[variant + "_rng_next"] = np.array(np.random.random())      # where the stream stands after the three scenes
    out = os.path.join(HERE, "augment.npz")
    np.savez_compressed(out, **gold)
    print("wrote augment.npz %.0f KB" % (os.path.getsize(out) / 1024))
