"""The ground-truth database of `gt_sampling`, cut on the GPU from scans that already live in HBM (csrc/gt_database.hip,
include/btcdet_hip_gtdb.h).

    frames = KittiFrames(root, "train", fov_points_only=False)
    db = GtDatabase.build(frames, used_classes=["Car", "Pedestrian", "Cyclist"])
    augmentor = DataAugmentor(root, cfgs, class_names, db_infos=db.db_infos)       # no kitti_dbinfos_train.pkl is read
    device_aug = DeviceAugmentor(augmentor, db.bank)                               # no gt_database/*.bin is opened
    db.save(root)                                                                  # the files the reference's sampler reads

What is replaced: KittiDataset.create_groundtruth_database (btcdet/datasets/kitti/kitti_dataset.py:267-317), whose point work is
roiaware_pool3d's compiled points_in_boxes_cpu.  Here the scans of a batch of frames go up in one copy (KittiFrames.load_batch with
crop=False: the reference cuts from the full scan), btc_cut_objects forms every object's rows in box-major order, and the host keeps
the reference's bookkeeping: names, paths, db_infos, by its own indexing.  The in-box test is database_sampler.points_in_boxes_mask bit
for bit -- the test by which gt_sampling later removes scan rows under a pasted box.

Not here: creating the info pickles (btcdet_amd/kitti_infos.py), Waymo, the ABLATION variants."""
import pathlib
import pickle

import numpy as np
import torch

from .device_augmentor import DeviceAugmentor, ObjectBank, removal_rows

ROW_BOX_LIMIT = 2 ** 31        # sum over the scenes of rows x boxes: what the kernel's int32 counters can hold in the worst case


def cut_layout(scene_offsets, boxes_per_scene, centres=None):
    """the host side of one btc_cut_objects call.  scene_offsets (B+1) ascending host ints; boxes_per_scene: B arrays (m_s, >= 7) as
    given (float64 in the infos); centres: B arrays (m_s, 3) or None = the boxes' own first three columns.
    -> dict: rows (m, 8) f32 from the float32 boxes (the reference passes boxes.float()), centre (m, 3) f64 from the boxes as given,
    box_offsets (B+1) i32, max_boxes, n, m.  Raises ValueError when sum_s rows_s * boxes_s reaches 2^31."""
    offs = np.asarray(scene_offsets, dtype=np.int64).reshape(-1)
    B = offs.shape[0] - 1
    if B < 1 or len(boxes_per_scene) != B:
        raise ValueError("cut_layout: %d scene offsets for %d box arrays" % (offs.shape[0], len(boxes_per_scene)))
    if offs[0] != 0 or np.any(np.diff(offs) < 0) or offs[-1] >= 2 ** 31:
        raise ValueError("cut_layout: scene offsets must start at 0, ascend and fit 31 bits")
    boxes = [np.asarray(b) for b in boxes_per_scene]
    if any(b.ndim != 2 or b.shape[1] < 7 for b in boxes):
        raise ValueError("cut_layout: boxes are (m, >= 7) arrays: x, y, z, dx, dy, dz, heading")
    counts = np.array([b.shape[0] for b in boxes], dtype=np.int64)
    work = int((np.diff(offs) * counts).sum())
    if work >= ROW_BOX_LIMIT:
        raise ValueError("cut_layout: %d (row, box) pairs in one batch reach 2^31: cut fewer frames per batch" % work)
    if centres is None:
        centres = [b[:, 0:3] for b in boxes]
    rows = [removal_rows(b[:, 0:7].astype(np.float32)) for b in boxes if b.shape[0]]
    ctr = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in centres]
    if [c.shape[0] for c in ctr] != counts.tolist():
        raise ValueError("cut_layout: one centre per box")
    return {"rows": np.concatenate(rows, axis=0) if rows else np.zeros((0, 8), np.float32),
            "centre": np.ascontiguousarray(np.concatenate(ctr, axis=0)) if ctr else np.zeros((0, 3), np.float64),
            "box_offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), "max_boxes": int(counts.max()),
            "n": int(offs[-1]), "m": int(counts.sum()), "scene_offsets": offs.astype(np.int32)}


def second_capacity(total, capacity):
    """the rows of the second btc_cut_objects call, or None when the first one held everything: the first call offers as many rows as
    the scans have (a row inside two boxes appears twice, so the total can exceed it), and obj_offsets is true either way"""
    return int(total) if total > capacity else None


def cut_objects(points, scene_offsets, boxes_per_scene, centres=None, want_src=False):
    """btc_cut_objects on a resident batch.  points (n, ld) f32 on the GPU, scenes contiguous; scene_offsets (B+1) host ints (a tensor
    is read back); boxes_per_scene / centres as cut_layout takes them.
    -> (rows (total, ld) f32 on the GPU, box-major; obj_offsets (m+1) host int64 [; src_idx (total) device i32, the source rows])
    One staging copy up, one (m+1)-int read-back (the host needs num_points_in_gt anyway), a second call only when total > n."""
    from ._lib import check, lib, ptr, stream_ptr, workspace
    L, dev = lib(), points.device
    if isinstance(scene_offsets, torch.Tensor):
        scene_offsets = scene_offsets.cpu().numpy()
    lay = cut_layout(scene_offsets, boxes_per_scene, centres)
    points = points.contiguous()
    n, ld = points.shape
    if n != lay["n"]:
        raise ValueError("cut_objects: %d rows, scene offsets end at %d" % (n, lay["n"]))
    B, m, max_boxes = len(boxes_per_scene), lay["m"], lay["max_boxes"]
    boxes, centre, box_offs, offs = DeviceAugmentor._upload([lay["rows"], lay["centre"], lay["box_offsets"], lay["scene_offsets"]], dev)
    obj_offs = torch.empty((m + 1,), dtype=torch.int32, device=dev)
    ws_bytes = L.btc_cut_objects_ws_bytes(n, B, m, max_boxes)
    ws = workspace(ws_bytes, dev)

    def call(cap):
        out = torch.empty((cap, ld), dtype=torch.float32, device=dev)
        src = torch.empty((cap,), dtype=torch.int32, device=dev) if want_src else None
        check(L.btc_cut_objects(ptr(points) if n else None, n, ld, ptr(offs), B, ptr(boxes) if m else None, ptr(centre) if m else None,
                                ptr(box_offs), m, max_boxes, cap, ptr(out) if cap else None, ptr(obj_offs), ptr(src) if (want_src and cap) else None,
                                ptr(ws), ws_bytes, stream_ptr()), "btc_cut_objects")
        return out, src, obj_offs.cpu().numpy().astype(np.int64)

    out, src, bounds = call(n)
    again = second_capacity(bounds[-1], n)
    if again is not None:
        out, src, bounds = call(again)
    total = int(bounds[-1])
    return (out[:total], bounds, src[:total]) if want_src else (out[:total], bounds)


class GtDatabase(object):
    """the result of build(): db_infos (class name -> list of the reference's db_info dicts, in its order), bank (an ObjectBank over
    rows that never left the device; its table holds every object's path, used class or not), num_points (per object, in file
    order), objects (path, first_row, n_rows per written file, in the reference's order)."""

    def __init__(self, split, num_point_features):
        self.split, self.num_point_features = split, int(num_point_features)
        self.db_infos, self.objects, self.bank = {}, [], None

    @property
    def num_points(self):
        return np.array([n for _, _, n in self.objects], dtype=np.int64)

    @staticmethod
    def database_dir(split):
        return "gt_database" if split == "train" else "gt_database_%s" % split

    @staticmethod
    def frame_boxes(info):
        """an info's gt_boxes_lidar (None for a frame without annos); a KeyError names the frame"""
        if "annos" not in info:
            return None
        if "gt_boxes_lidar" not in info["annos"]:
            raise KeyError("frame %s: its annos have no gt_boxes_lidar (the infos were written without the lidar boxes)"
                           % info["point_cloud"]["lidar_idx"])
        return info["annos"]["gt_boxes_lidar"]

    def add_frame(self, info, counts, first):
        """kitti_dataset.py:279-312 for one frame whose objects hold counts[i] rows from row `first` on: object i takes names[i],
        difficulty[i], bbox[i], score[i] by the SAME index into the unfiltered anno arrays; every object gets a file entry, only
        used classes a db_info.  -> the row behind the frame's last object"""
        sample_idx = info["point_cloud"]["lidar_idx"]
        annos = info["annos"]
        names, difficulty, bbox, gt_boxes = annos["name"], annos["difficulty"], annos["bbox"], annos["gt_boxes_lidar"]
        for i in range(gt_boxes.shape[0]):
            path = str(pathlib.Path(self.database_dir(self.split)) / ("%s_%s_%d.bin" % (sample_idx, names[i], i)))
            self.objects.append((path, int(first), int(counts[i])))
            if (self.used_classes is None) or names[i] in self.used_classes:
                db_info = {"name": names[i], "path": path, "image_idx": sample_idx, "gt_idx": i, "box3d_lidar": gt_boxes[i],
                           "num_points_in_gt": int(counts[i]), "difficulty": difficulty[i], "bbox": bbox[i], "score": annos["score"][i]}
                self.db_infos.setdefault(names[i], []).append(db_info)
            first += int(counts[i])
        return first

    @classmethod
    def from_arrays(cls, infos, objects_per_frame, split="train", used_classes=None, num_point_features=4):
        """the bookkeeping of build() over host arrays: objects_per_frame[k] = the list of (n_i, F) arrays of info k's objects (ignored
        for an info without annos).  What the CPU tests and a host-made database go through."""
        self = cls(split, num_point_features)
        self.used_classes = used_classes
        parts, first = [], 0
        annotated = [cls.frame_boxes(info) is not None for info in infos]      # every frame is looked at before any is cut, as in build()
        for info, objs, has in zip(infos, objects_per_frame, annotated):
            if not has:
                continue
            first = self.add_frame(info, [o.shape[0] for o in objs], first)
            parts.extend(np.asarray(o, np.float32).reshape(-1, self.num_point_features) for o in objs)
        rows = np.concatenate(parts, axis=0) if parts else np.zeros((0, self.num_point_features), np.float32)
        self.bank = ObjectBank.from_rows(rows, {p: (f, n) for p, f, n in self.objects}, self.num_point_features)
        return self

    @classmethod
    def build(cls, frames, used_classes=None, frames_per_batch=16, device="cuda"):
        """frames: a KittiFrames.  Walks it frames_per_batch at a time: the raw scans up in one copy, one cut, one read-back of the
        objects' sizes.  A frame without annos is skipped (the reference raises a KeyError there)."""
        self = cls(frames.split, frames.NUM_POINT_FEATURES)
        self.used_classes = used_classes
        todo = [k for k in range(len(frames)) if cls.frame_boxes(frames.infos[k]) is not None]
        pieces, first = [], 0
        for at in range(0, len(todo), max(int(frames_per_batch), 1)):
            idx = todo[at:at + max(int(frames_per_batch), 1)]
            batch = frames.load_batch(idx, device, crop=False)
            offs = np.concatenate([[0], np.cumsum(batch["raw_rows"])])
            rows, bounds = cut_objects(batch["points"], offs, [frames.infos[k]["annos"]["gt_boxes_lidar"] for k in idx])
            pieces.append(rows)
            counts, j = np.diff(bounds), 0
            for k in idx:
                m_k = frames.infos[k]["annos"]["gt_boxes_lidar"].shape[0]
                first = self.add_frame(frames.infos[k], counts[j:j + m_k], first)
                j += m_k
        if first >= 2 ** 31:
            raise ValueError("GtDatabase.build: %d object rows do not fit 31 bits" % first)
        dev_rows = torch.cat(pieces, dim=0) if pieces else torch.zeros((0, self.num_point_features), dtype=torch.float32, device=device)
        self.bank = ObjectBank.from_rows(None, {p: (f, n) for p, f, n in self.objects}, self.num_point_features, device_rows=dev_rows)
        return self

    def save(self, root, split=None):
        """writes <root>/gt_database[_<split>]/*.bin and <root>/kitti_dbinfos_<split>.pkl: what the reference's DataBaseSampler and the
        file-reading ObjectBank(root, db_infos) read back.  The paths in db_infos name the directory of the split it was built for."""
        split = self.split if split is None else split
        if split != self.split:
            raise ValueError("the database was built for split %r: its paths name %s" % (self.split, self.database_dir(self.split)))
        root = pathlib.Path(root)
        (root / self.database_dir(split)).mkdir(parents=True, exist_ok=True)
        rows = self.bank.rows
        for path, first, n in self.objects:
            with open(root / path, "wb") as f:
                f.write(np.ascontiguousarray(rows[first:first + n]).tobytes())
        with open(root / ("kitti_dbinfos_%s.pkl" % split), "wb") as f:
            pickle.dump(self.db_infos, f)
        return root / ("kitti_dbinfos_%s.pkl" % split)
