"""Golden vectors of the reference's best-match step inside its training augmentation (runs only where the reference is mounted): its
OWN DataAugmentor.forward (btcdet/datasets/augmentor/data_augmentor.py:171-202) with its own DataBaseSampler, its own
MltBestMatchQuerier (multi_best_match_querier.py) and augmentor_utils, queue gt_sampling -> add_multi_best_match -> the world
transforms in both shipped orders (tests/best_match_cases.py), over the database, the three scenes and the seeded template pickles
named there, global numpy RNG seeded with 99.  The DataAugmentor is made with object.__new__ and its queue set by hand, as
gen_augment_golden.py does; the two compiled primitives the sampler calls are served by the restatements of gen_sampler_golden.py.

Every output key of every scene is recorded: `bm_points` and the host keys in full, the other point arrays as shape + SHA-1.  The
generator asserts that gt_boxes is float32 when the best-match step runs: otherwise the device route would not be the one under test.

    python tests/golden/gen_best_match_golden.py   ->  tests/golden/best_match.npz"""
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gen_sampler_golden as gs  # noqa: E402  (installs the stubs and the two restated primitives, imports the reference's sampler)
import augment_cases as ac  # noqa: E402
import best_match_cases as bc  # noqa: E402
import common  # noqa: E402
from btcdet.datasets.augmentor.data_augmentor import DataAugmentor  # noqa: E402
from btcdet.datasets.augmentor.multi_best_match_querier import MltBestMatchQuerier  # noqa: E402


def float32_boxes(step):
    def run(data_dict):
        assert data_dict["gt_boxes"].dtype == np.float32, data_dict["gt_boxes"].dtype
        return step(data_dict=data_dict)
    return run


if __name__ == "__main__":
    gold = {}
    for order in bc.ORDERS:
        with tempfile.TemporaryDirectory() as d:
            infos = common.make_gt_database(d)
            bc.write_templates(Path(d), bc.templates(infos))
            aug = object.__new__(DataAugmentor)
            aug.root_path, aug.class_names, aug.db_infos, aug.logger = Path(d), ac.CLASSES, infos, None
            aug.data_augmentor_queue = []
            for cfg in bc.queue_cfgs(order):
                if cfg.NAME == "gt_sampling":
                    aug.data_augmentor_queue.append(gs.DataBaseSampler(Path(d), cfg, ac.CLASSES, infos))
                elif cfg.NAME == "add_multi_best_match":
                    step = aug.add_multi_best_match(config=cfg)
                    assert type(step) is MltBestMatchQuerier
                    aug.data_augmentor_queue.append(float32_boxes(step))
                else:
                    aug.data_augmentor_queue.append(getattr(aug, cfg.NAME)(config=cfg))
            np.random.seed(ac.SEED)
            for i, sc in enumerate(bc.scenes()):
                r = aug.forward(sc)
                assert r["bm_points"].dtype == np.float32
                ac.record(gold, "%s%d_" % (order, i), r, full=False)
                print(order, i, r["points"].shape, r["gt_boxes"].shape, r.get("augment_box_num"), r["bm_points"].shape, sorted(r))
            gold[order + "_rng_next"] = np.array(np.random.random())      # where the stream stands after the three scenes
    out = os.path.join(HERE, "best_match.npz")
    np.savez_compressed(out, **gold)
    print("wrote best_match.npz %.0f KB" % (os.path.getsize(out) / 1024))
