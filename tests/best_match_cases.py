"""Inputs shared by the best-match golden generator (tests/golden/gen_best_match_golden.py) and the tests that consume its vectors
(tests/test_best_match_cpu.py, tests/test_hip_best_match.py, tests/test_hip_best_match_abi_contract.py): the three scenes and the
database of tests/augment_cases.py with a frame id each, `add_multi_best_match` between the sampler and the world transforms in both
shipped queue orders, seeded templates of 20-60 rows for every box the step can meet, and the numpy restatement of
include/btcdet_hip_bestmatch.h.  Imports nothing that needs a GPU."""
import pickle

import numpy as np

import augment_cases as ac

ORDERS = {"model": "model_w0", "dataset": "dataset_w0"}      # queue order -> the variant of augment_cases it extends
FRAME_IDS = ("000007", "000008", "000009")
DIRS = {"Car": "bm_car", "Cyclist": "bm_cyc", "Pedestrian": "bm_ped"}
TEMPLATE_SEED = 17


def bm_cfg():
    return ac.ED(NAME="add_multi_best_match", CAR_MLT_BM_ROOT=DIRS["Car"], CYC_MLT_BM_ROOT=DIRS["Cyclist"], PED_MLT_BM_ROOT=DIRS["Pedestrian"],
                 LOAD_POINT_FEATURES=3)


def queue_cfgs(order):
    q = ac.queue_cfgs(ORDERS[order])
    return [q[0], bm_cfg()] + q[1:]


def scenes():
    out = ac.scenes()
    for sc, frame in zip(out, FRAME_IDS):
        sc["frame_id"] = frame
    return out


def templates(infos):
    """(class, image_idx, gt_idx) -> (n, 3) float32, n in [20, 60]: one per database object and one per box of every scene"""
    keys = [(name, int(e["image_idx"]), int(e["gt_idx"])) for name in sorted(infos) for e in infos[name]]
    for sc in scenes():
        keys += [("Car", int(sc["frame_id"]), i) for i in range(sc["gt_boxes"].shape[0])]
    rng = np.random.default_rng(TEMPLATE_SEED)
    return {k: rng.uniform(-2, 2, (int(rng.integers(20, 61)), 3)).astype(np.float32) for k in keys}


def write_templates(root, arrays):
    """the arrays as the reference's pickles (a flat float array per file) -> template_root (class name -> directory)"""
    roots = {name: root / d for name, d in DIRS.items() if name != "Cyclist"}
    for r in roots.values():
        r.mkdir(exist_ok=True)
    for (name, img, gt), a in arrays.items():
        with open(roots[name] / "{}_{}.pkl".format(img, gt), "wb") as f:
            pickle.dump(a.reshape(-1), f)
    return roots


def build(tmp_path, order):
    """-> (DataAugmentor with the best-match step, ObjectBank, template arrays, template_root) over fresh files under tmp_path"""
    from btcdet_amd.device_augmentor import DataAugmentor, ObjectBank
    infos = ac.common.make_gt_database(tmp_path)
    arrays = templates(infos)
    roots = write_templates(tmp_path, arrays)
    aug = DataAugmentor(tmp_path, ac.ED(DISABLE_AUG_LIST=["placeholder"], AUG_CONFIG_LIST=queue_cfgs(order)), ac.CLASSES, db_infos=infos)
    return aug, ObjectBank(tmp_path, infos, 4), arrays, roots


# ------------------------------------------------------------------------------------- include/btcdet_hip_bestmatch.h in numpy
def restate_rows(t, place):
    """template rows (n, 3) float32 placed by `place` = c, ms, s, cx, cy, cz: every product and sum a float32 operation of its own,
    accumulated from +0 in the order np.einsum("nj,ij->ni", t, R) + centre takes"""
    c, ms, s, cx, cy, cz = (np.float32(v) for v in place[:6])
    zero, one = np.float32(0), np.float32(1)
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    return np.stack([(((zero + x * c) + y * ms) + z * zero) + cx,
                     (((zero + x * s) + y * c) + z * zero) + cy,
                     (((zero + x * zero) + y * zero) + z * one) + cz], axis=1).astype(np.float32)


def restate_place_templates(bank, first, rows, place, bm_offsets, ops, op_offsets, out_ld=3):
    """btc_place_templates in numpy -> (n_out, out_ld) float32; a row outside the bank is zeros (the scene column stays)"""
    out = []
    for b in range(len(bm_offsets) - 1):
        sc_ops = np.asarray(ops, np.float32).reshape(-1, 4)[op_offsets[b]:op_offsets[b + 1]]
        n_set = 0 if (len(sc_ops) and sc_ops[0][3] != 0) else 45      # the op's flag names the rotation form
        for p in range(bm_offsets[b], bm_offsets[b + 1]):
            src = int(first[p]) + np.arange(int(rows[p]), dtype=np.int64)
            ok = (src >= 0) & (src < bank.shape[0]) & (int(first[p]) >= 0)
            xyz = np.zeros((int(rows[p]), 3), np.float32)
            if ok.any():
                xyz[ok] = ac.restate_ops(restate_rows(bank[src[ok]], place[p]), sc_ops, n_set)[0]
            out.append(xyz if out_ld == 3 else np.concatenate([np.full((xyz.shape[0], 1), b, np.float32), xyz], axis=1))
    return np.concatenate(out, axis=0) if out else np.zeros((0, out_ld), np.float32)
