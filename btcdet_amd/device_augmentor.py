"""Training augmentation: the reference's DataAugmentor protocol on the host, and the same augmentation applied to a batch of raw
scans that already lives in HBM (csrc/augment.hip, include/btcdet_hip_augment.h).

  DataAugmentor     btcdet/datasets/augmentor/data_augmentor.py:9-202 over the functions this package already has
                    (database_sampler.DataBaseSampler, data_side.random_flip_along_x / global_scaling / random_world_rotation /
                    best_match_points): the queue from AUG_CONFIG_LIST minus DISABLE_AUG_LIST in the configured order, `forward`
                    with the reference's bookkeeping.  Per-scene numpy: what a DataLoader worker runs, and what the device path is
                    compared with (tests/test_augment_cpu.py pins it to the reference's own class, tests/golden/augment.npz).
  ObjectBank        every database object's .bin loaded once into one (sum n_i, F) array, `path -> (first_row, n_rows)`.
  TemplateBank      every best-match template's .pkl loaded once into one (sum n_i, 3) array, `(class, image_idx, gt_idx) ->
                    (first_row, n_rows)`: with one, plan() turns the add_multi_best_match step into placements (template rows, yaw
                    rotation, box centre) and apply() forms `bm_points` in one launch from the resident bank
                    (csrc/best_match.hip, include/btcdet_hip_bestmatch.h) -- no file is opened and no point formed on the host.
  DeviceAugmentor   plan(scenes): host only, O(boxes) -- runs the augmentor's queue on the boxes of every scene of the batch with the
                    same sampler object, consuming the global numpy RNG exactly as DataAugmentor.forward would for these scenes
                    back to back, and records what the points need: removal boxes, pasted objects, the op program.  It reads no
                    point.  apply(points, scene_offsets, plan): the HIP kernels; the output is what
                    DataProcessor.forward_raw_batch takes.

RNG.  plan() draws what DataAugmentor.forward draws for scene 0, then scene 1, ...  The reference's __getitem__ interleaves every
scene's shuffle permutation (data_processor.py:41-51) between them: the stream is the reference's DataAugmentor.forward stream, not
its whole __getitem__ stream.  Permutations are handed to DataProcessor.mask_and_shuffle_batch(shuffle_idx=...) afterwards."""
import pathlib
import pickle
import re

import numpy as np
import torch

from . import data_side, database_sampler
from .data_side import SPECIAL_NAMES

AUG_FLIP_X, AUG_SCALE, AUG_ROT, AUG_MAX_OPS = 1, 2, 3, 8     # include/btcdet_hip_augment.h
SMALL_SET = 45                                               # rotate_points_along_z: 9 n < 400
WORLD_STEPS = ("random_world_flip", "random_world_scaling", "random_world_rotation")


def _get(cfg, key, default=None):
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


def limit_period(val, offset=0.5, period=np.pi):
    """common_utils.limit_period on a numpy array: float32 torch arithmetic, like the reference's check_numpy_to_torch"""
    t = torch.from_numpy(np.ascontiguousarray(val)).float()
    return (t - torch.floor(t / period + offset) * period).numpy()


def _special(data_dict):
    names = [k for k in SPECIAL_NAMES if k in data_dict]
    return names, [data_dict[k] for k in names]


class _WorldFlip(object):
    def __init__(self, config):
        for axis in config["ALONG_AXIS_LIST"]:
            assert axis in ["x", "y"]
            if axis == "y":
                raise NotImplementedError("random_world_flip along y: data_side has no random_flip_along_y")
        self.config = config

    def __call__(self, data_dict):
        gt_boxes, points = data_dict["gt_boxes"], data_dict["points"]
        names, special = _special(data_dict)
        for _ in self.config["ALONG_AXIS_LIST"]:
            gt_boxes, points, special = data_side.random_flip_along_x(gt_boxes, points, special_points_lst=special, enable=None)
        data_dict.update(zip(names, special))
        data_dict["gt_boxes"], data_dict["points"] = gt_boxes, points
        return data_dict


class _WorldScaling(object):
    def __init__(self, config):
        self.config = config

    def __call__(self, data_dict):
        names, special = _special(data_dict)
        gt_boxes, points, special = data_side.global_scaling(data_dict["gt_boxes"], data_dict["points"], self.config["WORLD_SCALE_RANGE"],
                                                             special_points_lst=special)
        data_dict.update(zip(names, special))
        data_dict["gt_boxes"], data_dict["points"] = gt_boxes, points
        return data_dict


class _WorldRotation(object):
    def __init__(self, config):
        self.config = config

    def __call__(self, data_dict):
        return data_side.random_world_rotation(data_dict, self.config)


class MltBestMatchQuerier(object):
    """MltBestMatchQuerier.__call__ (multi_best_match_querier.py:50-98,278-296) without ABLATION: `bm_points` = the best-match templates
    of the scene's own boxes (data_side.best_match_points) and of the boxes the sampler pasted.  template_root: class name -> directory."""

    def __init__(self, template_root, config, class_names):
        if _get(config, "ABLATION") is not None:
            raise NotImplementedError("add_multi_best_match with ABLATION")
        self.template_root, self.config, self.class_names = template_root, config, class_names
        self.load_point_features = _get(config, "LOAD_POINT_FEATURES", 3)

    def __call__(self, data_dict):
        n_aug = data_dict["aug_boxes_image_idx"].shape[0] if "aug_boxes_image_idx" in data_dict else 0
        boxes, names = data_dict["gt_boxes"], data_dict["gt_names"]
        n_own = boxes.shape[0] - n_aug
        assert n_own == data_dict["gt_boxes_inds"].shape[0]
        parts = []
        own = data_side.best_match_points(boxes[:n_own], names[:n_own], data_dict["gt_boxes_inds"], data_dict["frame_id"], self.template_root,
                                          self.class_names, self.load_point_features)
        if own.shape[0] > 0:
            parts.append(own)
        if n_aug and "pre_aug_bm" not in data_dict:
            for k in range(n_aug):
                box, name = boxes[n_own + k], names[n_own + k]
                t = data_side.read_bm_template(self.template_root[name] / "{}_{}.pkl".format(data_dict["aug_boxes_image_idx"][k],
                                                                                             data_dict["aug_boxes_gt_idx"][k]), self.load_point_features)
                parts.append(np.einsum("nj,ij->ni", t, data_side.get_yaw_rotation(box[6])) + box[:3])
        if len(parts) > 1:
            data_dict["bm_points"] = np.concatenate(parts, axis=0)[..., :3]
        elif len(parts) == 1:
            data_dict["bm_points"] = parts[0][..., :3]
        else:
            data_dict["bm_points"] = np.zeros([0, 3], dtype=np.float32)
        return data_dict


class DataAugmentor(object):
    def __init__(self, root_path, augmentor_configs, class_names, logger=None, db_infos=None, template_root=None):
        self.root_path = pathlib.Path(root_path)
        self.class_names, self.logger, self.template_root = class_names, logger, template_root
        self.db_infos = db_infos if db_infos is not None else {}
        self.data_augmentor_queue, self.queue_names, self.queue_configs = [], [], []
        is_list = isinstance(augmentor_configs, list)
        for cfg in (augmentor_configs if is_list else augmentor_configs["AUG_CONFIG_LIST"]):
            name = cfg["NAME"]
            if not is_list and name in augmentor_configs["DISABLE_AUG_LIST"]:
                continue
            maker = {"gt_sampling": self.gt_sampling, "add_multi_best_match": self.add_multi_best_match, "random_world_flip": _WorldFlip,
                     "random_world_rotation": _WorldRotation, "random_world_scaling": _WorldScaling}.get(name)
            if maker is None:
                raise NotImplementedError("augmentor step %r" % name)
            self.data_augmentor_queue.append(maker(cfg))
            self.queue_names.append(name)
            self.queue_configs.append(cfg)

    def _load_db_infos(self, config):
        if len(self.db_infos) == 0:
            for name in self.class_names:
                self.db_infos[name] = []
            for rel in config["DB_INFO_PATH"]:
                with open(str(self.root_path.resolve() / rel), "rb") as f:
                    infos = pickle.load(f)
                for name in self.class_names:
                    self.db_infos[name].extend(infos[name])

    def gt_sampling(self, config):
        self._load_db_infos(config)
        return database_sampler.DataBaseSampler(root_path=self.root_path, sampler_cfg=config, class_names=self.class_names,
                                                db_infos=self.db_infos, logger=self.logger)

    def add_multi_best_match(self, config):
        root = self.template_root
        if root is None:
            base = self.root_path.resolve()
            root = {"Car": base / config["CAR_MLT_BM_ROOT"], "Cyclist": base / config["CYC_MLT_BM_ROOT"], "Pedestrian": base / config["PED_MLT_BM_ROOT"]}
        return MltBestMatchQuerier(root, config, self.class_names)

    def __getstate__(self):
        d = dict(self.__dict__)
        del d["logger"]
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)
        self.logger = None

    def finish(self, data_dict):
        """what forward does behind the queue"""
        data_dict["gt_boxes"][:, 6] = limit_period(data_dict["gt_boxes"][:, 6], offset=0.5, period=2 * np.pi)
        if "road_plane" in data_dict:
            data_dict.pop("road_plane")
        if "gt_boxes_mask" in data_dict:
            mask = data_dict["gt_boxes_mask"]
            data_dict["gt_boxes"] = data_dict["gt_boxes"][mask]
            data_dict["gt_names"] = data_dict["gt_names"][mask]
            if "obj_ids" in data_dict:
                data_dict["obj_ids"] = data_dict["obj_ids"][mask]
            data_dict.pop("gt_boxes_mask")
        data_dict.pop("gt_boxes_inds", None)
        return data_dict

    def forward(self, data_dict, validation=False):
        """points (N, 3 + C), gt_boxes (M, 7 + C), gt_names (M), gt_boxes_mask (M) [, road_plane, calib, frame_id]"""
        data_dict["gt_boxes_inds"] = np.arange(list(data_dict["gt_boxes_mask"].shape)[0])
        for step in self.data_augmentor_queue:
            if not validation or isinstance(step, MltBestMatchQuerier):
                data_dict = step(data_dict)
        return self.finish(data_dict)


class ObjectBank(object):
    """every object of a ground-truth database in one array: rows (sum n_i, F) float32, table path -> (first_row, n_rows).
    ObjectBank(root, db_infos, F) reads one file per object; from_rows takes rows that exist already, on the host or on the device."""

    def __init__(self, root_path, db_infos, num_point_features):
        root = pathlib.Path(root_path)
        self.num_point_features = int(num_point_features)
        self.table, parts, first = {}, [], 0
        for entries in db_infos.values():
            for e in entries:
                if e["path"] in self.table:
                    continue
                obj = np.fromfile(str(root / e["path"]), dtype=np.float32).reshape([-1, self.num_point_features])
                self.table[e["path"]] = (first, obj.shape[0])
                parts.append(obj)
                first += obj.shape[0]
        self.rows = np.concatenate(parts, axis=0) if parts else np.zeros((0, self.num_point_features), np.float32)
        self._device = {}

    @classmethod
    def from_rows(cls, rows, table, num_point_features, device_rows=None):
        """a bank from rows that are already in one array; reads no file.  rows (sum n_i, F) float32 on the host, or None with
        device_rows: a (sum n_i, F) float32 tensor that is the bank on its device (gt_database.GtDatabase: the rows never left it) --
        tensor() of that device returns it, and `rows` is copied from it on first host access."""
        self = cls.__new__(cls)
        self.num_point_features = int(num_point_features)
        self.table = dict(table)
        self._device, self._resident = {}, None
        if device_rows is not None:
            assert device_rows.dtype == torch.float32 and device_rows.dim() == 2 and device_rows.shape[1] == self.num_point_features
            self._resident = device_rows.contiguous()
        if rows is not None:
            self.rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.num_point_features)
            assert self._resident is None or self._resident.shape[0] == self.rows.shape[0]
        elif self._resident is None:
            raise ValueError("ObjectBank.from_rows: neither rows nor device_rows")
        n_rows = self._resident.shape[0] if rows is None else self.rows.shape[0]
        assert all(0 <= f and n >= 0 and f + n <= n_rows for f, n in self.table.values()), "a table entry outside the rows"
        return self

    @property
    def rows(self):
        if self._rows is None:
            self._rows = self._resident.cpu().numpy()
        return self._rows

    @rows.setter
    def rows(self, value):
        self._rows = value

    _rows = None
    _resident = None

    def tensor(self, device):
        res = self._resident
        if res is not None:
            want = torch.device(device)
            if want.type == res.device.type and want.index in (None, res.device.index):
                return res
        key = str(device)
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.rows).to(device).contiguous()
        return self._device[key]


class TemplateBank(object):
    """every best-match template under `template_root` (class name -> directory of <image_idx>_<gt_idx>.pkl) in one array: rows
    (sum n_i, 3) float32 as data_side.read_bm_template gives them, table (class name, image_idx, gt_idx) -> (first_row, n_rows).
    keys: an iterable of such triples restricts loading to them (a missing one raises KeyError).  Read once; nothing is known about the
    size of a real bank, so `nbytes` is there to be looked at before tensor() uploads it."""
    _NAME = re.compile(r"^(\d+)_(\d+)\.pkl$")

    def __init__(self, template_root, load_point_features=3, keys=None):
        self.load_point_features = int(load_point_features)
        found = {}
        for name in sorted(template_root):
            directory = pathlib.Path(template_root[name])
            for path in sorted(directory.iterdir()) if directory.is_dir() else ():
                m = self._NAME.match(path.name)
                if m:
                    found[(str(name), int(m.group(1)), int(m.group(2)))] = path
        if keys is not None:
            wanted = [(str(n), int(i), int(g)) for n, i, g in keys]
            for k in wanted:
                if k not in found:
                    raise KeyError("best-match template %s" % (pathlib.Path(template_root[k[0]]) / "{}_{}.pkl".format(k[1], k[2])))
            found = {k: found[k] for k in sorted(set(wanted))}
        self._fill({k: data_side.read_bm_template(path, self.load_point_features) for k, path in found.items()})

    @classmethod
    def from_arrays(cls, arrays, load_point_features=3):
        """arrays: (class name, image_idx, gt_idx) -> (n, 3) float32 rows; reads no file (tests, synthetic data)"""
        self = cls.__new__(cls)
        self.load_point_features = int(load_point_features)
        self._fill({(str(n), int(i), int(g)): np.asarray(a, dtype=np.float32).reshape(-1, 3) for (n, i, g), a in arrays.items()})
        return self

    def _fill(self, arrays):
        self.table, parts, first = {}, [], 0
        for k in sorted(arrays):
            self.table[k] = (first, arrays[k].shape[0])
            parts.append(arrays[k])
            first += arrays[k].shape[0]
        assert first < 2 ** 31, "template rows are addressed with int32"
        self.rows = np.ascontiguousarray(np.concatenate(parts, axis=0), dtype=np.float32) if parts else np.zeros((0, 3), np.float32)
        self._device = {}

    @classmethod
    def from_rows(cls, rows, table, device_rows=None, load_point_features=3):
        """a bank from rows that are already in one array, beside ObjectBank.from_rows; reads no file.  table: (class name, image_idx,
        gt_idx) -> (first_row, n_rows).  rows (sum n_i, 3) float32 on the host, or None with device_rows: a (sum n_i, 3) float32 tensor
        that is the bank on its device (template_builder.TemplateBuilder: the rows never left it) -- tensor() of that device returns
        it, and `rows` is copied from it on first host access."""
        self = cls.__new__(cls)
        self.load_point_features = int(load_point_features)
        self.table = {(str(n), int(i), int(g)): (int(f), int(c)) for (n, i, g), (f, c) in table.items()}
        self._device, self._resident = {}, None
        if device_rows is not None:
            assert device_rows.dtype == torch.float32 and device_rows.dim() == 2 and device_rows.shape[1] == 3
            self._resident = device_rows.contiguous()
        if rows is not None:
            self.rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 3)
            assert self._resident is None or self._resident.shape[0] == self.rows.shape[0]
        elif self._resident is None:
            raise ValueError("TemplateBank.from_rows: neither rows nor device_rows")
        n_rows = self._resident.shape[0] if rows is None else self.rows.shape[0]
        assert n_rows < 2 ** 31, "template rows are addressed with int32"
        assert all(0 <= f and n >= 0 and f + n <= n_rows for f, n in self.table.values()), "a table entry outside the rows"
        return self

    @property
    def rows(self):
        if self._rows is None:
            self._rows = self._resident.cpu().numpy()
        return self._rows

    @rows.setter
    def rows(self, value):
        self._rows = value

    _rows = None
    _resident = None

    @property
    def nbytes(self):
        res = self._resident
        return int(self.rows.nbytes) if res is None else int(res.numel() * res.element_size())

    def tensor(self, device):
        res = self._resident
        if res is not None:
            want = torch.device(device)
            if want.type == res.device.type and want.index in (None, res.device.index):
                return res
        key = str(device)
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.rows).to(device).contiguous()
        return self._device[key]


class AugPlan(object):
    """what DeviceAugmentor.plan leaves for apply: flat numpy arrays in the layout of btc_augment_batch, and the host keys per scene"""
    ARRAYS = ("rm_boxes", "rm_offsets", "obj_first", "obj_rows", "obj_shift", "obj_offsets", "ops", "op_offsets", "rot_z")
    # the layout of btc_place_templates (include/btcdet_hip_bestmatch.h): one placement per box the best-match step serves, in the
    # host step's order -- bm_first / bm_rows (P) i32 the template's rows in the TemplateBank, bm_place (P, 8) f32 c, ms, s, cx, cy, cz,
    # 0, 0, bm_offsets (B+1) i32 placements per scene, bm_row_offsets (P+1) i32 the prefix of bm_rows; bm_rows_total its last entry.
    # bm_device[b]: scene b's bm_points come from placements (its ops rows then carry the small-set flag of ITS bm_points in column
    # 3, which btc_augment_batch ignores); otherwise from special[b]["bm_points"], made on the host
    BM_ARRAYS = ("bm_first", "bm_rows", "bm_place", "bm_offsets", "bm_row_offsets")

    def __init__(self, batch):
        self.batch = batch
        self.scenes = []          # the host keys of every scene as DataAugmentor.forward leaves them (no point arrays)
        self.special = []         # per scene: name -> (n, 3) float32 sets made on the host by the queue (bm_points), untransformed
        self.save_pre_rot = False


class DeviceAugmentor(object):
    def __init__(self, augmentor, bank, templates=None):
        self.augmentor, self.bank, self.templates = augmentor, bank, templates
        names = augmentor.queue_names
        for step in augmentor.data_augmentor_queue:
            if templates is not None and isinstance(step, MltBestMatchQuerier):
                assert step.load_point_features == templates.load_point_features, "the bank was read with another LOAD_POINT_FEATURES"
        if "gt_sampling" in names and any(n in WORLD_STEPS for n in names[:names.index("gt_sampling")]):
            raise NotImplementedError("gt_sampling behind a world transform: the kernels remove and paste first")
        if sum(n == "gt_sampling" for n in names) > 1:
            raise NotImplementedError("more than one gt_sampling step")
        if sum(n in WORLD_STEPS for n in names) > AUG_MAX_OPS:
            raise NotImplementedError("more than %d world transforms" % AUG_MAX_OPS)
        rot = [c for n, c in zip(names, augmentor.queue_configs) if n == "random_world_rotation"]
        self.save_pre_rot = bool(rot) and bool(_get(rot[0], "SAVE_PRE_ROT", False))

    # ------------------------------------------------------------------------------------------------------------------ host
    def _plan_paste(self, sampler, rec):
        """stands in for DataBaseSampler._paste while the plan runs: the same box bookkeeping, the points left to the device"""
        def paste(data_dict, new_boxes, new_entries):
            keep = data_dict["gt_boxes_mask"]
            boxes, names = data_dict["gt_boxes"][keep], data_dict["gt_names"][keep]
            data_dict["gt_boxes_inds"] = data_dict["gt_boxes_inds"][keep]
            lift = None
            if sampler.sampler_cfg.get("USE_ROAD_PLANE", False):
                new_boxes, lift = sampler.put_boxes_on_road_planes(new_boxes, data_dict["road_plane"], data_dict["calib"])
                data_dict.pop("calib")
                data_dict.pop("road_plane")
            for i, e in enumerate(new_entries):
                first, n = self.bank.table[e["path"]]
                c = e["box3d_lidar"]
                rec["objects"].append((first, n, float(c[0]), float(c[1]), float(c[2]), float(lift[i]) if lift is not None else 0.0))
            grown = np.array(new_boxes[:, 0:7], dtype=np.float32, copy=True)
            extra = sampler.sampler_cfg.REMOVE_EXTRA_WIDTH
            if sum(extra) > 1e-3:
                grown[:, 3:6] += np.asarray(extra, dtype=np.float32)[None, :]
            rec["rm_boxes"] = removal_rows(grown)
            new_names = np.array([e["name"] for e in new_entries])
            if boxes.ndim != 2 or boxes.shape[0] == 0:
                data_dict["gt_boxes"], data_dict["gt_names"] = new_boxes, new_names
            else:
                data_dict["gt_boxes"], data_dict["gt_names"] = np.concatenate([boxes, new_boxes], axis=0), np.concatenate([names, new_names], axis=0)
            data_dict["augment_box_num"] = new_boxes.shape[0]
            return data_dict
        return paste

    def _plan_best_match(self, step, d, placements):
        """stands in for MltBestMatchQuerier.__call__ while the plan runs: one placement per box the step would have served, in its
        order (the scene's own boxes of an in-scope class, then the pasted ones), no file opened, no point formed -> rows placed"""
        n_aug = d["aug_boxes_image_idx"].shape[0] if "aug_boxes_image_idx" in d else 0
        boxes, names = d["gt_boxes"], d["gt_names"]
        n_own = boxes.shape[0] - n_aug
        assert n_own == d["gt_boxes_inds"].shape[0]
        image_idx = int(d["frame_id"])
        served = [(i, image_idx, d["gt_boxes_inds"][i]) for i in range(n_own) if names[i] in step.class_names]
        if n_aug and "pre_aug_bm" not in d:
            served += [(n_own + k, d["aug_boxes_image_idx"][k], d["aug_boxes_gt_idx"][k]) for k in range(n_aug)]
        total = 0
        for i, img, gt in served:
            name = names[i]
            hit = self.templates.table.get((str(name), int(img), int(gt)))
            if hit is None:
                raise KeyError("best-match template %s is not in the TemplateBank" % (step.template_root[name] / "{}_{}.pkl".format(img, gt)))
            yaw = boxes[i][6]                                  # a float32 scalar: the expressions of data_side.get_yaw_rotation
            c, s = np.cos(yaw), np.sin(yaw)
            ms = -1.0 * s
            assert c.dtype == ms.dtype == np.float32
            placements.append((hit[0], hit[1], (c, ms, s, boxes[i][0], boxes[i][1], boxes[i][2], 0.0, 0.0)))
            total += hit[1]
        return total

    def plan(self, scenes):
        """scenes: list of dicts with gt_boxes, gt_names, gt_boxes_mask [, road_plane, calib, frame_id, ...]; a `points` key is ignored"""
        aug = self.augmentor
        plan = AugPlan(len(scenes))
        plan.save_pre_rot = self.save_pre_rot
        rm, rm_off, objs, obj_off, ops, op_off, rot_z = [], [0], [], [0], [], [0], []
        placements, bm_off, plan.bm_device = [], [0], []
        for scene in scenes:
            d = {k: v for k, v in scene.items() if k not in ("points", "pre_rot_points") and k not in SPECIAL_NAMES}
            d["gt_boxes_inds"] = np.arange(list(d["gt_boxes_mask"].shape)[0])
            rec = {"objects": [], "rm_boxes": np.zeros((0, 8), np.float32)}
            scene_ops, host_special, bm_placed = [], {}, None
            for name, step in zip(aug.queue_names, aug.data_augmentor_queue):
                # a probe point stands in for the scan: the step draws what it draws, transforms the boxes, and shows what it did
                if name == "gt_sampling":
                    d["points"] = np.zeros((0, self.bank.num_point_features), np.float32)
                    step._paste = self._plan_paste(step, rec)
                    try:
                        d = step(d)
                    finally:
                        del step._paste
                elif name == "add_multi_best_match" and self.templates is not None and d["gt_boxes"].dtype == np.float32:
                    bm_placed = self._plan_best_match(step, d, placements)
                elif name == "add_multi_best_match":
                    # without a bank -- or with boxes that are not float32, where the host chain works in float64 and has no single
                    # device form -- the step runs on the host and the set is uploaded
                    d = step(d)
                    host_special["bm_points"] = np.ascontiguousarray(d.pop("bm_points"), dtype=np.float32)
                elif name == "random_world_flip":
                    d["points"] = np.array([[0, 1, 0, 0]], np.float32)
                    d = step(d)
                    # one draw per listed axis, each along x: an odd number of flips is a flip
                    if d["points"][0, 1] < 0:
                        scene_ops.append((AUG_FLIP_X, 0.0, 0.0, 0.0))
                elif name == "random_world_scaling":
                    d["points"] = np.ones((1, 4), np.float32)
                    d = step(d)
                    r = step.config["WORLD_SCALE_RANGE"]
                    if not r[1] - r[0] < 1e-3:
                        scene_ops.append((AUG_SCALE, d["points"][0, 0], 0.0, 0.0))      # float32(noise_scale): the probe times it
                elif name == "random_world_rotation":
                    d["points"] = np.array([[1, 0, 0, 0]], np.float32)
                    d = step(d)
                    scene_ops.append((AUG_ROT, d["points"][0, 0], d["points"][0, 1], 0.0))   # cos, sin as rotate_points_along_z made them
            d = aug.finish(d)
            for k in ("points", "pre_rot_points"):
                d.pop(k, None)
            rot_z.append(np.float32(d["rot_z"]) if "rot_z" in d else np.float32(0))
            plan.scenes.append(d)
            plan.special.append(host_special)
            rm.append(rec["rm_boxes"])
            rm_off.append(rm_off[-1] + rec["rm_boxes"].shape[0])
            objs.extend(rec["objects"])
            obj_off.append(len(objs))
            plan.bm_device.append(bm_placed is not None)
            bm_off.append(len(placements))
            if bm_placed is not None:      # the rotation form of the scene's bm_points, known here: the kernel takes it from the op
                scene_ops = [op[:3] + (1.0 if bm_placed < SMALL_SET else 0.0,) for op in scene_ops]
            ops.extend(scene_ops)
            op_off.append(len(ops))
        o = np.array(objs, dtype=np.float64).reshape(-1, 6)
        plan.rm_boxes = np.concatenate(rm, axis=0).astype(np.float32) if rm else np.zeros((0, 8), np.float32)
        plan.rm_offsets = np.array(rm_off, np.int32)
        plan.obj_first, plan.obj_rows = o[:, 0].astype(np.int32), o[:, 1].astype(np.int32)
        plan.obj_shift = np.ascontiguousarray(o[:, 2:6])
        plan.obj_offsets = np.array(obj_off, np.int32)
        plan.ops = np.array(ops, dtype=np.float32).reshape(-1, 4)
        plan.op_offsets = np.array(op_off, np.int32)
        plan.rot_z = np.array(rot_z, np.float32)
        plan.paste_rows = int(plan.obj_rows.sum())
        plan.bm_first = np.array([p[0] for p in placements], np.int32)
        plan.bm_rows = np.array([p[1] for p in placements], np.int32)
        plan.bm_place = np.array([p[2] for p in placements], np.float32).reshape(-1, 8)
        plan.bm_offsets = np.array(bm_off, np.int32)
        row_off = np.concatenate([[0], np.cumsum(plan.bm_rows, dtype=np.int64)])
        assert row_off[-1] < 2 ** 31, "bm_points rows of a batch are addressed with int32"
        plan.bm_row_offsets = row_off.astype(np.int32)
        plan.bm_rows_total = int(plan.bm_row_offsets[-1])
        return plan

    # ---------------------------------------------------------------------------------------------------------------- device
    @staticmethod
    def _upload(arrays, device):
        """numpy arrays -> device tensors through ONE pinned buffer and one asynchronous copy (no synchronisation; the caching
        host allocator keeps the pinned block until the copy has run)"""
        spans, off = [], 0
        for a in arrays:
            spans.append((off, a.nbytes))
            off += max((a.nbytes + 255) // 256 * 256, 256)      # an empty array still gets an address
        host = torch.empty((max(off, 256),), dtype=torch.uint8).pin_memory()
        view = host.numpy()
        for a, (o, nb) in zip(arrays, spans):
            view[o:o + nb] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        dev = host.to(device, non_blocking=True)
        out = []
        for a, (o, nb) in zip(arrays, spans):
            t = dev[o:o + max(nb, a.dtype.itemsize)].view(_TORCH_DTYPE[a.dtype.name])
            out.append(t[:a.size].view(a.shape) if a.size else t[:0].view(a.shape))
        return out

    def apply(self, points, scene_offsets, plan, special=None, sync=True, indexed_bm=False):
        """points (sum N, F) f32 raw scans on the GPU, scenes contiguous; scene_offsets (B+1) i32; special: name -> (stacked (sum n, 3) f32
        device tensor, offsets (B+1) host ints) of sets in data_side.SPECIAL_NAMES: they get the scene's flip, scale and rotation.
        -> dict: points, pre_rot_points (iff SAVE_PRE_ROT), scene_offsets (device i32), rot_z (device f32 degrees, iff SAVE_PRE_ROT),
        special (name -> (tensor, offsets)), and the plan's host keys as lists over the scenes (gt_boxes, gt_names, ...).
        sync=True trims the point outputs after one (B+1)-int read-back and adds scene_counts; sync=False reads nothing back: the
        point outputs keep their capacity (N + pasted rows) and scene_offsets[B] on the device says how many rows are valid.
        A plan made with a TemplateBank: special["bm_points"] is formed from the bank by btc_place_templates (its offsets are known on
        the host: no read-back either way); indexed_bm=True adds `bm_points`, the (n, 4) [scene, x, y, z] form collate gives the
        key, from the same launch -- special["bm_points"][0] is then the (n, 3) view of its last three columns."""
        from ._lib import check, lib, ptr, stream_ptr, workspace
        L, dev = lib(), points.device
        B = plan.batch
        points = points.contiguous()
        n, ld = points.shape
        assert scene_offsets.numel() == B + 1, "one plan entry per scene"
        assert ld == self.bank.num_point_features or plan.paste_rows == 0, "scan rows and database rows differ in width"
        offs = scene_offsets if (scene_offsets.is_cuda and scene_offsets.dtype == torch.int32) else \
            scene_offsets.to(torch.int32).pin_memory().to(dev, non_blocking=True)
        bm_device = any(getattr(plan, "bm_device", ()))
        up = self._upload([getattr(plan, k) for k in AugPlan.ARRAYS + (AugPlan.BM_ARRAYS if bm_device else ())], dev)
        (rm_boxes, rm_offsets, obj_first, obj_rows, obj_shift, obj_offsets, ops, op_offsets, rot_z) = up[:len(AugPlan.ARRAYS)]
        bank = self.bank.tensor(dev)
        cap = n + plan.paste_rows
        out = torch.empty((cap, ld), dtype=torch.float32, device=dev)
        out_pre = torch.empty((cap, ld), dtype=torch.float32, device=dev) if plan.save_pre_rot else None
        new_offs = torch.empty((B + 1,), dtype=torch.int32, device=dev)
        n_obj = int(plan.obj_first.shape[0])
        ws_bytes = L.btc_augment_ws_bytes(n, B, n_obj)
        ws = workspace(ws_bytes, dev)
        check(L.btc_augment_batch(ptr(points) if n else None, n, ld, ptr(offs), B, ptr(rm_boxes) if plan.rm_boxes.size else None, ptr(rm_offsets),
                                  ptr(bank) if n_obj else None, bank.shape[0], ptr(obj_first), ptr(obj_rows), ptr(obj_shift), ptr(obj_offsets), n_obj,
                                  plan.paste_rows, ptr(ops) if plan.ops.size else None, ptr(op_offsets), cap, ptr(out) if cap else None,
                                  ptr(out_pre) if (out_pre is not None and cap) else None, ptr(new_offs), ptr(ws), ws_bytes, stream_ptr()),
              "btc_augment_batch")
        res = {"scene_offsets": new_offs}
        # the special sets: the op program alone, the rotation form from their (host-known) sizes
        sets = dict(special or {})
        for name in SPECIAL_NAMES:
            if any(name in s for s in plan.special):
                assert name not in sets, "%s comes from the plan's queue and from the caller" % name
                parts = [s.get(name, np.zeros((0, 3), np.float32)) for s in plan.special]
                stacked = np.concatenate(parts, axis=0)
                (t,) = self._upload([stacked], dev)
                sets[name] = (t, np.cumsum([0] + [p.shape[0] for p in parts]))
        res["special"] = {}
        for name, (t, set_offs) in sets.items():
            assert name in SPECIAL_NAMES, name
            so = np.asarray(set_offs.cpu() if isinstance(set_offs, torch.Tensor) else set_offs).astype(np.int32)
            assert so.shape[0] == B + 1 and so[-1] == t.shape[0]
            sp_ops = plan.ops.copy()
            for b in range(B):
                sp_ops[plan.op_offsets[b]:plan.op_offsets[b + 1], 3] = 1.0 if so[b + 1] - so[b] < SMALL_SET else 0.0
            d_so, d_ops = self._upload([so, sp_ops], dev)
            t = t.contiguous()
            o = torch.empty_like(t)
            check(L.btc_world_transform(ptr(t) if t.shape[0] else None, t.shape[0], t.shape[1], ptr(d_so), B, ptr(d_ops) if sp_ops.size else None,
                                        ptr(op_offsets), ptr(o) if t.shape[0] else None, stream_ptr()), "btc_world_transform")
            res["special"][name] = (o, so)
        if bm_device:
            assert special is None or "bm_points" not in special, "bm_points comes from the plan's placements and from the caller"
            placed, placed_offs = self._place_templates(plan, up[len(AugPlan.ARRAYS):], ops, op_offsets, 4 if indexed_bm else 3, dev)
            if "bm_points" in res["special"]:      # some scenes took the host route: per scene, in scene order
                hosted, hosted_offs = res["special"]["bm_points"]
                if indexed_bm:
                    col = torch.repeat_interleave(torch.arange(B, dtype=torch.float32), torch.from_numpy(np.diff(hosted_offs).astype(np.int64)))
                    hosted = torch.cat([col.to(dev, non_blocking=True)[:, None], hosted], dim=1)
                parts = [(placed[placed_offs[b]:placed_offs[b + 1]] if plan.bm_device[b] else hosted[hosted_offs[b]:hosted_offs[b + 1]]) for b in range(B)]
                placed = torch.cat(parts, dim=0)
                placed_offs = np.cumsum([0] + [p.shape[0] for p in parts]).astype(np.int32)
            if indexed_bm:
                res["bm_points"] = placed
            res["special"]["bm_points"] = (placed[:, 1:] if indexed_bm else placed, placed_offs)
        elif indexed_bm:
            raise ValueError("indexed_bm=True needs a plan whose bm_points come from a TemplateBank")
        for k in sorted({k for s in plan.scenes for k in s}):
            res[k] = [s.get(k) for s in plan.scenes]
        if plan.save_pre_rot:
            res["rot_z"] = rot_z
        if sync:
            bounds = new_offs.tolist()
            res["scene_counts"] = [bounds[b + 1] - bounds[b] for b in range(B)]
            out = out[:bounds[B]]
            out_pre = out_pre[:bounds[B]] if out_pre is not None else None
        res["points"] = out
        if out_pre is not None:
            res["pre_rot_points"] = out_pre
        return res


    def _place_templates(self, plan, bm_arrays, ops, op_offsets, out_ld, dev):
        """btc_place_templates over the plan's placements -> ((bm_rows_total, out_ld) tensor, (B+1) host offsets of the scenes' rows)"""
        from ._lib import check, lib, ptr, stream_ptr
        bm_first, bm_rows, bm_place, bm_offsets, bm_row_offsets = bm_arrays
        bank = self.templates.tensor(dev)
        n_pl, n_out = int(plan.bm_first.shape[0]), plan.bm_rows_total
        out = torch.empty((n_out, out_ld), dtype=torch.float32, device=dev)
        check(lib().btc_place_templates(ptr(bank) if n_pl else None, bank.shape[0], ptr(bm_first) if n_pl else None, ptr(bm_rows) if n_pl else None,
                                        ptr(bm_place) if n_pl else None, ptr(bm_offsets), ptr(bm_row_offsets), n_pl, plan.batch,
                                        ptr(ops) if plan.ops.size else None, ptr(op_offsets), n_out, out_ld, ptr(out) if n_out else None, stream_ptr()),
              "btc_place_templates")
        return out, plan.bm_row_offsets[plan.bm_offsets]


_TORCH_DTYPE = {"float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "uint8": torch.uint8}


def removal_rows(boxes):
    """(M, 7) boxes -> (M, 8) float32 rows of btc_augment_batch: centre, dx/2 + margin, dy/2 + margin, dz/2, cos(-heading), sin(-heading),
    every value by the expression database_sampler.points_in_boxes_mask forms it with (margin 1e-2)"""
    b = np.asarray(boxes, dtype=np.float32)
    margin = np.float32(1e-2)
    c, s = np.cos(-b[:, 6]).astype(np.float32), np.sin(-b[:, 6]).astype(np.float32)
    return np.stack([b[:, 0], b[:, 1], b[:, 2], b[:, 3] / np.float32(2.0) + margin, b[:, 4] / np.float32(2.0) + margin, b[:, 5] / np.float32(2.0),
                     c, s], axis=1).astype(np.float32)
