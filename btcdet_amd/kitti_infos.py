"""The KITTI info pickles, made from the raw directory: labels, image shapes, calibrations, lidar boxes, the points in every
ground-truth box and the coverage rates (csrc/kitti_infos.hip, include/btcdet_hip_infos.h).

    create_kitti_infos(root)                                  # kitti_infos_{train,val,test}.pkl, gt_database[_val]/, kitti_dbinfos_*.pkl
    create_kitti_infos_with_coverage(root, template_roots)    # kitti_cvrg_infos_{train,val}.pkl

    infos = KittiInfoBuilder(root, "train").get_infos()       # the list KittiDataset.get_infos returns
    infos = add_coverage(infos, db.bank, templates, "train")  # + annos["coverage_rates"], from banks that live in HBM

What is replaced: the reference's KittiDataset.get_infos (btcdet/datasets/kitti/kitti_dataset.py:129-201), create_kitti_infos,
create_info_file_with_coverage (204-264) and create_kitti_infos_with_coverage.  ImageSets/, training/{velodyne,calib,label_2,image_2}
and testing/ are all that is read.

What runs where: labels, PNG headers, calibrations and dictionaries are host work, in the reference's numpy statements so that every
field has its dtype and bits.  num_points_in_gt -- lidar_to_rect, get_fov_flag and a Delaunay in_hull per box over ~120 K rows per
scan -- is btc_count_in_boxes over the raw scans KittiFrames.load_batch(crop=False) uploads, with one (m + batch)-int read-back per
batch.  The unique-cell counts of get_coords are btc_coverage_cells over the rows of a TemplateBank and of GtDatabase.bank: one
launch for every object of a split, one read-back.

Not here: reading image pixels (the shape comes from the PNG header), Waymo, the `trainval` infos (the reference has them commented
out)."""
import logging
import pathlib
import pickle
import struct

import numpy as np

from .kitti_frames import CALIB_FLOATS, Calibration, KittiFrames

log = logging.getLogger(__name__)
COVERAGE_CLASSES = ("Car", "Pedestrian", "Cyclist")
SPHERE_RES = (0.32, 0.5184, 0.4203125)       # sphere_coords_res of create_info_file_with_coverage
COVERAGE_LDS_ROWS = 4096                      # BTC_COVERAGE_LDS_KEYS / 2: a job of more rows takes a table in the workspace
COVERAGE_OK, COVERAGE_WIDE, COVERAGE_BAD = 0, 1, 2
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
ROW_BOX_LIMIT = 2 ** 31                       # sum over the scenes of rows x boxes: what an int32 count can hold in the worst case


# ------------------------------------------------------------------------------------------------------------------------ labels
class Object3d(object):
    """one line of a label_2 file: the fields of the reference's object3d_kitti.Object3d that get_infos reads, with its types (box2d
    and loc float32 arrays, the rest Python floats) and its difficulty rule"""

    def __init__(self, line):
        label = line.strip().split(" ")
        self.src = line
        self.cls_type = label[0]
        self.truncation, self.occlusion, self.alpha = float(label[1]), float(label[2]), float(label[3])
        self.box2d = np.array((float(label[4]), float(label[5]), float(label[6]), float(label[7])), dtype=np.float32)
        self.h, self.w, self.l = float(label[8]), float(label[9]), float(label[10])
        self.loc = np.array((float(label[11]), float(label[12]), float(label[13])), dtype=np.float32)
        self.ry = float(label[14])
        self.score = float(label[15]) if len(label) == 16 else -1.0
        self.level = self.get_kitti_obj_level()

    def get_kitti_obj_level(self):
        height = float(self.box2d[3]) - float(self.box2d[1]) + 1
        if height >= 40 and self.truncation <= 0.15 and self.occlusion <= 0:
            return 0      # Easy
        if height >= 25 and self.truncation <= 0.3 and self.occlusion <= 1:
            return 1      # Moderate
        if height >= 25 and self.truncation <= 0.5 and self.occlusion <= 2:
            return 2      # Hard
        return -1


def get_objects_from_label(label_file):
    with open(label_file, "r") as f:
        return [Object3d(line) for line in f.readlines()]


def image_shape(path):
    """(H, W) int32 of a PNG, from its IHDR chunk: 24 bytes are read, nothing is decoded"""
    with open(path, "rb") as f:
        head = f.read(24)
    if len(head) < 24 or head[:8] != PNG_SIGNATURE or head[12:16] != b"IHDR":
        raise ValueError("%s: not a PNG file (no signature and IHDR chunk in its first 24 bytes)" % path)
    w, h = struct.unpack(">II", head[16:24])
    return np.array([h, w], dtype=np.int32)


def annotations_of(obj_list, calib):
    """kitti_dataset.py:153-177: the annos of one frame without num_points_in_gt, every array by the reference's expression"""
    if not obj_list:
        raise ValueError("a label file without objects (the reference cannot concatenate an empty list either)")
    a = {}
    a["name"] = np.array([obj.cls_type for obj in obj_list])
    a["truncated"] = np.array([obj.truncation for obj in obj_list])
    a["occluded"] = np.array([obj.occlusion for obj in obj_list])
    a["alpha"] = np.array([obj.alpha for obj in obj_list])
    a["bbox"] = np.concatenate([obj.box2d.reshape(1, 4) for obj in obj_list], axis=0)
    a["dimensions"] = np.array([[obj.l, obj.h, obj.w] for obj in obj_list])      # lhw (camera) format
    a["location"] = np.concatenate([obj.loc.reshape(1, 3) for obj in obj_list], axis=0)
    a["rotation_y"] = np.array([obj.ry for obj in obj_list])
    a["score"] = np.array([obj.score for obj in obj_list])
    a["difficulty"] = np.array([obj.level for obj in obj_list], np.int32)
    num_objects = len([obj.cls_type for obj in obj_list if obj.cls_type != "DontCare"])
    num_gt = len(a["name"])
    a["index"] = np.array(list(range(num_objects)) + [-1] * (num_gt - num_objects), dtype=np.int32)
    loc, dims, rots = a["location"][:num_objects], a["dimensions"][:num_objects], a["rotation_y"][:num_objects]
    loc_lidar = calib.rect_to_lidar(loc)
    l, h, w = dims[:, 0:1], dims[:, 1:2], dims[:, 2:3]
    loc_lidar[:, 2] += h[:, 0] / 2
    a["gt_boxes_lidar"] = np.concatenate([loc_lidar, l, w, h, -(np.pi / 2 + rots[..., np.newaxis])], axis=1)
    return a


def calib_info(calib):
    """kitti_dataset.py:142-147: the three 4 x 4 matrices, with the dtypes the reference's concatenations give (P2 and
    Tr_velo_to_cam float64, R0_rect float32)"""
    P2 = np.concatenate([calib.P2, np.array([[0., 0., 0., 1.]])], axis=0)
    R0_4x4 = np.zeros([4, 4], dtype=calib.R0.dtype)
    R0_4x4[3, 3] = 1.
    R0_4x4[:3, :3] = calib.R0
    V2C_4x4 = np.concatenate([calib.V2C, np.array([[0., 0., 0., 1.]])], axis=0)
    return {"P2": P2, "R0_rect": R0_4x4, "Tr_velo_to_cam": V2C_4x4}


# ------------------------------------------------------------------------------------------------------------- points in the boxes
def hull_rows(boxes):
    """(M, >= 7) boxes -> (M, 8) float32 rows of btc_count_in_boxes: centre, dx/2, dy/2, dz/2, cos(-heading), sin(-heading), every
    value formed in float32 from the float32 box: device_augmentor.removal_rows without the 0.01 margin (in_hull tests the bare hull)"""
    b = np.asarray(boxes)[:, 0:7].astype(np.float32)
    half = np.float32(2.0)
    c, s = np.cos(-b[:, 6]).astype(np.float32), np.sin(-b[:, 6]).astype(np.float32)
    return np.stack([b[:, 0], b[:, 1], b[:, 2], b[:, 3] / half, b[:, 4] / half, b[:, 5] / half, c, s], axis=1).astype(np.float32)


def count_in_boxes(points, scene_offsets, calib_blocks, boxes_per_scene, want_fov_rows=True):
    """btc_count_in_boxes on a resident batch.  points (n, ld) f32 on the GPU; scene_offsets (B+1) host ints; calib_blocks (B, 32) f32
    host; boxes_per_scene: B arrays (m_s, >= 7) as the infos hold them.
    -> (counts (m) host int32, fov_rows (B) host int32 or None): one staging copy up, ONE (m + B)-int read-back"""
    import torch
    from ._lib import check, lib, ptr, stream_ptr, workspace
    from .device_augmentor import DeviceAugmentor
    L, dev = lib(), points.device
    offs = np.asarray(scene_offsets, dtype=np.int64).reshape(-1)
    B = offs.shape[0] - 1
    points = points.contiguous()
    n, ld = points.shape
    if B < 1 or len(boxes_per_scene) != B or calib_blocks.shape != (B, CALIB_FLOATS):
        raise ValueError("count_in_boxes: %d scene offsets, %d box arrays, calibration blocks %r" % (offs.shape[0], len(boxes_per_scene), calib_blocks.shape))
    if offs[0] != 0 or np.any(np.diff(offs) < 0) or offs[-1] != n or n >= 2 ** 31:
        raise ValueError("count_in_boxes: scene offsets must start at 0, ascend and end at the %d rows" % n)
    per = np.array([np.asarray(b).shape[0] for b in boxes_per_scene], dtype=np.int64)
    if int((np.diff(offs) * per).sum()) >= ROW_BOX_LIMIT:
        raise ValueError("count_in_boxes: the (row, box) pairs of one batch reach 2^31: count fewer frames per batch")
    rows = [hull_rows(b) for b in boxes_per_scene if np.asarray(b).shape[0]]
    rows = np.concatenate(rows, axis=0) if rows else np.zeros((0, 8), np.float32)
    m = int(per.sum())
    box_offs = np.concatenate([[0], np.cumsum(per)]).astype(np.int32)
    d_rows, d_calib, d_box_offs, d_offs = DeviceAugmentor._upload([rows, np.ascontiguousarray(calib_blocks, np.float32), box_offs, offs.astype(np.int32)], dev)
    res = torch.empty((m + B,), dtype=torch.int32, device=dev)
    ws_bytes = L.btc_count_in_boxes_ws_bytes(n, B)
    ws = workspace(ws_bytes, dev)
    fov = res[m:] if want_fov_rows else None
    check(L.btc_count_in_boxes(ptr(points) if n else None, n, ld, ptr(d_offs), B, ptr(d_calib), ptr(d_rows) if m else None, ptr(d_box_offs), m,
                               ptr(res) if m else None, fov.data_ptr() if fov is not None else None, ptr(ws), ws_bytes, stream_ptr()),
          "btc_count_in_boxes")
    host = res.cpu().numpy()
    return host[:m].copy(), (host[m:].copy() if want_fov_rows else None)


class KittiInfoBuilder(object):
    """KittiInfoBuilder(root, split): get_infos() of the reference's KittiDataset set to `split`"""

    def __init__(self, root, split):
        self.root, self.split = pathlib.Path(root), split
        self.split_dir = self.root / ("training" if split != "test" else "testing")
        ids = self.root / "ImageSets" / (split + ".txt")
        self.sample_id_list = [x.strip() for x in open(ids).readlines()] if ids.exists() else None

    def frame_info(self, sample_idx, has_label=True):
        """process_single_scene without the point counts -> (info, calib)"""
        info = {"point_cloud": {"num_features": 4, "lidar_idx": sample_idx}}
        info["image"] = {"image_idx": sample_idx, "image_shape": image_shape(self.split_dir / "image_2" / ("%s.png" % sample_idx))}
        calib = Calibration(self.split_dir / "calib" / ("%s.txt" % sample_idx))
        info["calib"] = calib_info(calib)
        if has_label:
            label_file = self.split_dir / "label_2" / ("%s.txt" % sample_idx)
            try:
                info["annos"] = annotations_of(get_objects_from_label(label_file), calib)
            except ValueError as e:
                raise ValueError("%s: %s" % (label_file, e))
        return info

    def get_infos(self, has_label=True, count_inside_pts=True, sample_id_list=None, frames_per_batch=16, device="cuda"):
        """the list KittiDataset.get_infos returns.  With has_label and count_inside_pts the raw scans go up frames_per_batch at a time
        and btc_count_in_boxes fills annos["num_points_in_gt"] (int32, -1 for the DontCare rows); otherwise nothing runs on the GPU."""
        ids = list(sample_id_list if sample_id_list is not None else self.sample_id_list)
        infos = [self.frame_info(i, has_label) for i in ids]
        if not (has_label and count_inside_pts) or not infos:
            return infos
        frames = KittiFrames(self.root, self.split, fov_points_only=True, infos=infos)
        step = max(int(frames_per_batch), 1)
        for at in range(0, len(infos), step):
            idx = list(range(at, min(at + step, len(infos))))
            batch = frames.load_batch(idx, device, crop=False)
            offs = np.concatenate([[0], np.cumsum(batch["raw_rows"])])
            boxes = [infos[k]["annos"]["gt_boxes_lidar"] for k in idx]
            counts, _ = count_in_boxes(batch["points"], offs, frames.calib_blocks(idx), boxes, want_fov_rows=False)
            j = 0
            for k, b in zip(idx, boxes):
                annos = infos[k]["annos"]
                num = -np.ones(len(annos["name"]), dtype=np.int32)
                num[:b.shape[0]] = counts[j:j + b.shape[0]]
                annos["num_points_in_gt"] = num
                j += b.shape[0]
        return infos


# --------------------------------------------------------------------------------------------------------------------- coverage
def coverage_cells_host(tmpl, obj, box):
    """get_coords for one object in the reference's numpy statements (kitti_dataset.py:208-225, 246-251): tmpl (n, 3) f32 box-local,
    obj (k, >= 3) f32 centre-shifted, box (7) f64 -> (unique_obj, unique_bm).  The route of a job the kernel flags as too wide."""
    res = np.asarray([SPHERE_RES])

    def sphere(p):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        return np.stack([np.linalg.norm(p[:, :3], axis=1), np.arctan2(-y, x) * 180. / np.pi,
                         np.arctan2(z, np.linalg.norm(p[:, :2], axis=1)) * 180. / np.pi], axis=-1)

    box = np.asarray(box, np.float64)
    c, s = np.cos(box[6]), np.sin(box[6])
    rot = np.array([[c, -1.0 * s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    bm = np.einsum("nj,ij->ni", np.asarray(tmpl, np.float32).reshape(-1, 3), rot) + box[:3].reshape(-1, 3)
    if len(bm) == 0:
        return 0, 0
    sp = sphere(bm)
    mn = np.minimum(np.min(sp, axis=0), np.array([0.0, 0.0, 0.0])).reshape(1, 3)
    cells = np.floor_divide(sp - mn, res).astype(np.int32)
    n = np.max(cells, axis=0) + 11
    unique_bm = len(np.unique(cells, axis=0))
    pts = np.asarray(obj, np.float32)[:, :3] + box[:3].reshape(-1, 3)
    if len(pts) == 0:
        return 0, unique_bm
    cells = np.floor_divide(sphere(pts) - mn, res).astype(np.int32)
    keep = np.all(cells >= 0, axis=-1) & np.all(cells < n.reshape(1, 3), axis=-1)
    return len(np.unique(cells[keep], axis=0)), unique_bm


def coverage_cells(tmpl_rows, obj_rows, jobs, pose):
    """btc_coverage_cells.  tmpl_rows (T, 3), obj_rows (R, ld) f32 on the GPU; jobs (J, 4) int32, pose (J, 5) float64 on the host
    -> (cells (J, 2), status (J)) host int32.  Jobs of more than COVERAGE_LDS_ROWS rows go in a call of their own, so that only they
    size a workspace; one read-back per call."""
    import torch
    from ._lib import check, lib, ptr, stream_ptr, workspace
    from .device_augmentor import DeviceAugmentor
    L, dev = lib(), obj_rows.device
    jobs = np.ascontiguousarray(jobs, np.int32).reshape(-1, 4)
    pose = np.ascontiguousarray(pose, np.float64).reshape(-1, 5)
    J = jobs.shape[0]
    cells, status = np.zeros((J, 2), np.int32), np.zeros((J,), np.int32)
    tmpl_rows, obj_rows = tmpl_rows.contiguous(), obj_rows.contiguous()
    T, R, ld = tmpl_rows.shape[0], obj_rows.shape[0], obj_rows.shape[1]
    big = np.maximum(jobs[:, 1], jobs[:, 3]) > COVERAGE_LDS_ROWS
    for sel in (np.flatnonzero(~big), np.flatnonzero(big)):
        if sel.size == 0:
            continue
        max_rows = int(max(jobs[sel][:, [1, 3]].max(), 0))
        d_jobs, d_pose = DeviceAugmentor._upload([jobs[sel], pose[sel]], dev)
        res = torch.empty((3 * sel.size,), dtype=torch.int32, device=dev)
        ws_bytes = L.btc_coverage_cells_ws_bytes(int(sel.size), max_rows)
        if ws_bytes == 0:
            raise ValueError("coverage_cells: %d jobs of up to %d rows are refused" % (sel.size, max_rows))
        ws = workspace(ws_bytes, dev)
        check(L.btc_coverage_cells(ptr(tmpl_rows) if T else None, T, ptr(obj_rows) if R else None, R, ld, ptr(d_jobs), ptr(d_pose), int(sel.size),
                                   max_rows, ptr(res), res[2 * sel.size:].data_ptr(), ptr(ws), ws_bytes, stream_ptr()), "btc_coverage_cells")
        host = res.cpu().numpy()
        cells[sel], status[sel] = host[:2 * sel.size].reshape(-1, 2), host[2 * sel.size:]
    cells[status != COVERAGE_OK] = 0          # the kernel writes no counts for a flagged job
    return cells, status


def coverage_rate_array(rates):
    """the reference's shape quirk (kitti_dataset.py:254-259): (0, 1) float32 for no objects, (1, 1) for one, (n,) for more"""
    if len(rates) == 0:
        return np.zeros([0, 1], dtype=np.float32)
    if len(rates) == 1:
        return np.asarray(rates[0]).reshape(-1, 1)
    return np.stack(rates, axis=0)


def coverage_jobs(infos, bank, templates, split):
    """-> (jobs (J, 4) int32, pose (J, 5) float64, where [(info k, anno i)] per job); a missing template or database entry raises a
    KeyError that names it"""
    from .gt_database import GtDatabase
    jobs, pose, where = [], [], []
    for k, info in enumerate(infos):
        image_idx, annos = info["point_cloud"]["lidar_idx"], info["annos"]
        for i in range(len(annos["name"])):
            name = str(annos["name"][i])
            if name not in COVERAGE_CLASSES:
                continue
            key = (name, int(image_idx), i)
            path = str(pathlib.Path(GtDatabase.database_dir(split)) / ("%s_%s_%d.bin" % (image_idx, name, i)))
            if key not in templates.table:
                raise KeyError("frame %s object %d: no best-match template %s_%d.pkl of class %s" % (image_idx, i, int(image_idx), i, name))
            if path not in bank.table:
                raise KeyError("frame %s object %d: no database entry %s" % (image_idx, i, path))
            box = np.asarray(annos["gt_boxes_lidar"][i], np.float64)
            jobs.append(list(templates.table[key]) + list(bank.table[path]))
            pose.append([box[0], box[1], box[2], np.cos(box[6]), np.sin(box[6])])
            where.append((k, i))
    return np.array(jobs, np.int32).reshape(-1, 4), np.array(pose, np.float64).reshape(-1, 5), where


def add_coverage(infos, bank, templates, split, device="cuda", cells_fn=None):
    """the reference's create_info_file_with_coverage: sets info["annos"]["coverage_rates"] of every info (in place) and returns the
    list.  bank: an ObjectBank (GtDatabase.build(...).bank), templates: a TemplateBank keyed by (class, image_idx, gt_idx).  A name
    outside Car, Pedestrian, Cyclist gets 0.0; the others num_unique_obj / max(1, num_unique_bm), formed here in float64 from the two
    integers of btc_coverage_cells.  A job the kernel flags as wider than its key is computed by coverage_cells_host and logged.
    cells_fn(jobs, pose) -> (cells, status) replaces the kernel call (the CPU tests pass the numpy restatement)."""
    jobs, pose, where = coverage_jobs(infos, bank, templates, split)
    if cells_fn is not None:
        cells, status = cells_fn(jobs, pose)
    elif len(where):
        cells, status = coverage_cells(templates.tensor(device), bank.tensor(device), jobs, pose)
    else:
        cells, status = np.zeros((0, 2), np.int32), np.zeros((0,), np.int32)
    rates = {}
    for j, (k, i) in enumerate(where):
        if status[j] == COVERAGE_BAD:
            raise ValueError("frame %s object %d: its rows lie outside the banks" % (infos[k]["point_cloud"]["lidar_idx"], i))
        if status[j] == COVERAGE_WIDE:
            t0, tn, o0, on = (int(v) for v in jobs[j])
            log.warning("frame %s object %d: its cells do not fit the kernel's key, counted on the host", infos[k]["point_cloud"]["lidar_idx"], i)
            cells[j] = coverage_cells_host(templates.rows[t0:t0 + tn], bank.rows[o0:o0 + on], infos[k]["annos"]["gt_boxes_lidar"][i])
        rates[(k, i)] = int(cells[j, 0]) / max(1, int(cells[j, 1]))
    for k, info in enumerate(infos):
        info["annos"]["coverage_rates"] = coverage_rate_array([rates.get((k, i), 0.0) for i in range(len(info["annos"]["name"]))])
    return infos


# ------------------------------------------------------------------------------------------------------------------------ files
def create_kitti_infos(root, save_path=None, frames_per_batch=16, device="cuda"):
    """the reference's create_kitti_infos: kitti_infos_{train,val,test}.pkl under save_path (default: root), then the train and val
    ground-truth databases (every class) through GtDatabase.build(...).save(...).  -> {split: path}"""
    from .gt_database import GtDatabase
    root = pathlib.Path(root)
    save_path = root if save_path is None else pathlib.Path(save_path)
    paths, kept = {}, {}
    for split, has_label in (("train", True), ("val", True), ("test", False)):
        infos = KittiInfoBuilder(root, split).get_infos(has_label=has_label, count_inside_pts=has_label, frames_per_batch=frames_per_batch,
                                                        device=device)
        paths[split] = save_path / ("kitti_infos_%s.pkl" % split)
        with open(paths[split], "wb") as f:
            pickle.dump(infos, f)
        kept[split] = infos
    for split in ("train", "val"):
        frames = KittiFrames(root, split, fov_points_only=False, infos=kept[split])
        GtDatabase.build(frames, frames_per_batch=frames_per_batch, device=device).save(save_path)
    return paths


def create_kitti_infos_with_coverage(root, template_roots, save_path=None, frames_per_batch=16, device="cuda"):
    """the reference's create_kitti_infos_with_coverage: kitti_cvrg_infos_{train,val}.pkl from kitti_infos_{train,val}.pkl under
    save_path (default: root).  template_roots: class name -> directory of <image_idx>_<gt_idx>.pkl templates, or a TemplateBank.
    The database rows are cut again from the scans (GtDatabase.build) and never leave the device.  -> {split: path}"""
    from .device_augmentor import TemplateBank
    from .gt_database import GtDatabase
    root = pathlib.Path(root)
    save_path = root if save_path is None else pathlib.Path(save_path)
    templates = template_roots if isinstance(template_roots, TemplateBank) else TemplateBank(template_roots)
    paths = {}
    for split in ("train", "val"):
        with open(save_path / ("kitti_infos_%s.pkl" % split), "rb") as f:
            infos = pickle.load(f)
        frames = KittiFrames(root, split, fov_points_only=False, infos=infos)
        db = GtDatabase.build(frames, frames_per_batch=frames_per_batch, device=device)
        add_coverage(infos, db.bank, templates, split, device=device)
        paths[split] = save_path / ("kitti_cvrg_infos_%s.pkl" % split)
        with open(paths[split], "wb") as f:
            pickle.dump(infos, f)
    return paths
