"""KITTI frames for the resident pipeline: calibrations, the reference's info pickles, ground-truth boxes in the lidar frame, and raw
scans read straight into one pinned buffer, uploaded once and cropped to the camera's field of view on the GPU.

    frames = KittiFrames(root, "train")              # root/kitti_infos_train.pkl, root/training/{velodyne,calib,planes}
    scenes = [frames.scene(i) for i in idx]          # frame_id, calib, gt_names, gt_boxes [, road_plane], image_shape: the dict
                                                     # KittiDataset.__getitem__ hands to prepare_data (kitti_dataset.py:413-460), no points
    batch = frames.load_batch(idx, device)           # points (sum n', 4) f32 on the GPU, scene_offsets (B+1) device i32, scene_counts

What runs where: Calibration, scene() and the file reads are host work (O(boxes) and I/O); FOV_POINTS_ONLY -- lidar_to_rect, get_fov_flag,
points[fov_flag] over ~120 K rows per scan -- is btc_fov_crop (csrc/fov_crop.hip, include/btcdet_hip_frames.h), one stable compaction over
the batch.  fov_crop_host() is the same step in the reference's numpy statements.

Not here: reading image pixels (image shapes come from the infos), Waymo.  The info pickles are made by btcdet_amd/kitti_infos.py and
the ground-truth database is cut from these batches by btcdet_amd/gt_database.py.
"""
import copy
import os
import pathlib
import pickle

import numpy as np

CALIB_FLOATS = 32          # BTC_FOV_CALIB_FLOATS of include/btcdet_hip_frames.h


def _calib_arrays(path):
    """a KITTI calib/*.txt -> {"P2" (3, 4), "P3" (3, 4), "R0" (3, 3), "Tr_velo2cam" (3, 4)} float32: lines 2..5, the name dropped"""
    with open(path) as f:
        rows = [line.strip().split(" ")[1:] for line in f.readlines()[2:6]]
    p2, p3, r0, v2c = (np.array(r, dtype=np.float32) for r in rows)
    return {"P2": p2.reshape(3, 4), "P3": p3.reshape(3, 4), "R0": r0.reshape(3, 3), "Tr_velo2cam": v2c.reshape(3, 4)}


class Calibration(object):
    """Calibration(path | dict): the surface of the reference's calibration_kitti.Calibration (P2, R0, V2C and the frame changes), in the
    same numpy statements, so that float32 inputs give its bits on the same BLAS."""

    def __init__(self, calib_file):
        c = calib_file if isinstance(calib_file, dict) else _calib_arrays(calib_file)
        self.P2, self.R0, self.V2C = c["P2"], c["R0"], c["Tr_velo2cam"]
        self.cu, self.cv = self.P2[0, 2], self.P2[1, 2]
        self.fu, self.fv = self.P2[0, 0], self.P2[1, 1]
        self.tx, self.ty = self.P2[0, 3] / (-self.fu), self.P2[1, 3] / (-self.fv)

    def __getitem__(self, key):
        """calib["P2" | "R0" | "V2C" | "Tr_velo2cam"]: the dict form kitti_eval.prediction_anno reads"""
        return {"P2": self.P2, "R0": self.R0, "V2C": self.V2C, "Tr_velo2cam": self.V2C}[key]

    def cart_to_hom(self, pts):
        """(N, 3 | 2) -> (N, 4 | 3): a column of float32 ones appended"""
        return np.hstack((pts, np.ones((pts.shape[0], 1), dtype=np.float32)))

    def lidar_to_rect_matrix(self):
        """(4, 3) = np.dot(V2C.T, R0.T): the M of include/btcdet_hip_frames.h"""
        return np.dot(self.V2C.T, self.R0.T)

    def lidar_to_rect(self, pts_lidar):
        """(N, 3) lidar -> (N, 3) rectified camera frame"""
        return np.dot(self.cart_to_hom(pts_lidar), self.lidar_to_rect_matrix())

    def rect_to_lidar(self, pts_rect):
        """(N, 3) rectified camera frame -> (N, 3) lidar: the inverse of the 4 x 4 extension of R0 . V2C"""
        r0 = np.zeros((4, 4), dtype=np.float32)
        r0[:3, :3], r0[3, 3] = self.R0, 1
        v2c = np.zeros((4, 4), dtype=np.float32)
        v2c[:3, :], v2c[3, 3] = self.V2C, 1
        return np.dot(self.cart_to_hom(pts_rect), np.linalg.inv(np.dot(r0, v2c).T))[:, 0:3]

    def rect_to_img(self, pts_rect):
        """(N, 3) -> image points (N, 2) and the depth in the rectified camera frame (N)"""
        hom = self.cart_to_hom(pts_rect)
        img = np.dot(hom, self.P2.T)
        return (img[:, 0:2].T / hom[:, 2]).T, img[:, 2] - self.P2.T[3, 2]

    def lidar_to_img(self, pts_lidar):
        return self.rect_to_img(self.lidar_to_rect(pts_lidar))

    def img_to_rect(self, u, v, depth_rect):
        x = ((u - self.cu) * depth_rect) / self.fu + self.tx
        y = ((v - self.cv) * depth_rect) / self.fv + self.ty
        return np.concatenate((x.reshape(-1, 1), y.reshape(-1, 1), depth_rect.reshape(-1, 1)), axis=1)

    def corners3d_to_img_boxes(self, corners3d):
        """(N, 8, 3) corners in the rectified frame -> boxes (N, 4) [x1, y1, x2, y2] and the projected corners (N, 8, 2)"""
        hom = np.concatenate((corners3d, np.ones((corners3d.shape[0], 8, 1))), axis=2)
        img = np.matmul(hom, self.P2.T)
        x, y = img[:, :, 0] / img[:, :, 2], img[:, :, 1] / img[:, :, 2]
        boxes = np.stack((np.min(x, axis=1), np.min(y, axis=1), np.max(x, axis=1), np.max(y, axis=1)), axis=1)
        return boxes, np.stack((x, y), axis=2)


def get_fov_flag(pts_rect, img_shape, calib):
    """KittiDataset.get_fov_flag: inside the image (0 inclusive, width / height exclusive) and not behind the camera"""
    img, depth = calib.rect_to_img(pts_rect)
    in_u = np.logical_and(img[:, 0] >= 0, img[:, 0] < img_shape[1])
    in_v = np.logical_and(img[:, 1] >= 0, img[:, 1] < img_shape[0])
    return np.logical_and(np.logical_and(in_u, in_v), depth >= 0)


def boxes3d_kitti_camera_to_lidar(boxes3d_camera, calib):
    """(N, 7) [x, y, z, l, h, w, r] in the rectified camera frame (y the bottom face) -> (N, 7) lidar [x, y, z, dx, dy, dz, heading],
    z the centre"""
    l, h, w, r = (boxes3d_camera[:, k:k + 1] for k in (3, 4, 5, 6))
    xyz = calib.rect_to_lidar(boxes3d_camera[:, 0:3])
    xyz[:, 2] += h[:, 0] / 2
    return np.concatenate([xyz, l, w, h, -(r + np.pi / 2)], axis=-1)


def drop_info_with_name(info, name):
    keep = [i for i, x in enumerate(info["name"]) if x != name]
    return {key: info[key][keep] for key in info.keys()}


def read_road_plane(path):
    """planes/*.txt -> the unit plane (a, b, c, d) in the rectified camera frame with its normal facing up (b <= 0), float64; None
    without the file"""
    if not os.path.exists(path):
        return None
    with open(path, "r") as f:
        plane = np.asarray([float(v) for v in f.readlines()[3].split()])
    if plane[1] > 0:
        plane = -plane
    return plane / np.linalg.norm(plane[0:3])


def calib_block(calib, image_shape):
    """one scene's 32 floats of include/btcdet_hip_frames.h: M (4, 3), P2 (3, 4), W, H, six of padding"""
    h, w = int(image_shape[0]), int(image_shape[1])
    if not (0 <= h < 2 ** 24 and 0 <= w < 2 ** 24):
        raise ValueError("image shape %r: a side of 2^24 or more is not exact in float32" % (tuple(image_shape),))
    m, p2 = calib.lidar_to_rect_matrix(), calib.P2
    if m.dtype != np.float32 or p2.dtype != np.float32:
        raise ValueError("the calibration is not float32 (%s, %s): the crop is defined in float32" % (m.dtype, p2.dtype))
    block = np.zeros((CALIB_FLOATS,), np.float32)
    block[0:12], block[12:24], block[24], block[25] = m.reshape(-1), p2.reshape(-1), w, h
    return block


def fov_crop(points, scene_offsets, calib, out=None, keep_idx=None):
    """btc_fov_crop on resident arrays: points (n, ld) f32, scene_offsets (B+1) i32, calib (B, 32) f32, all on the GPU
    -> (out (n, ld) untrimmed, out_offsets (B+1) device i32); nothing is read back"""
    import torch
    from ._lib import check, lib, ptr, stream_ptr, workspace
    L, dev = lib(), points.device
    points = points.contiguous()
    n, ld = points.shape
    B = scene_offsets.numel() - 1
    offs = scene_offsets.to(device=dev, dtype=torch.int32).contiguous()
    if out is None:
        out = torch.empty_like(points)
    new_offs = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    ws_bytes = L.btc_fov_crop_ws_bytes(n, B)
    ws = workspace(ws_bytes, dev)
    check(L.btc_fov_crop(ptr(points), n, ld, ptr(offs), B, ptr(calib.contiguous()), out.shape[0], ptr(out), ptr(new_offs), ptr(keep_idx), ptr(ws),
                         ws_bytes, stream_ptr()), "btc_fov_crop")
    return out, new_offs


class KittiFrames(object):
    """KittiFrames(root, split, info_path=None, fov_points_only=True, infos=None): the frames of the reference's kitti_infos_<split>.pkl
    under `root` (the scans, calibrations and planes under root/training, root/testing for the test split), or of the list `infos`
    when it is given.  ImageSets/<split>.txt, when present, is read into sample_id_list.  fov_points_only is the data
    configuration's FOV_POINTS_ONLY: without it nothing is cropped."""
    NUM_POINT_FEATURES = 4

    def __init__(self, root, split, info_path=None, fov_points_only=True, infos=None):
        self.root, self.split, self.fov_points_only = pathlib.Path(root), split, bool(fov_points_only)
        self.split_dir = self.root / ("training" if split != "test" else "testing")
        ids = self.root / "ImageSets" / (split + ".txt")
        self.sample_id_list = [x.strip() for x in open(ids).readlines()] if ids.exists() else None
        if infos is not None:      # the list in memory (kitti_infos.KittiInfoBuilder: before any pickle exists); no file is opened
            self.infos = infos
        else:
            info_path = pathlib.Path(info_path) if info_path is not None else pathlib.Path("kitti_infos_%s.pkl" % split)
            with open(self.root / info_path, "rb") as f:
                self.infos = pickle.load(f)
        self._calibs = {}

    def __len__(self):
        return len(self.infos)

    # ------------------------------------------------------------------------------------------------------------------- per frame
    def frame_id(self, i):
        return self.infos[i]["point_cloud"]["lidar_idx"]

    def image_shape(self, i):
        return self.infos[i]["image"]["image_shape"]

    def calib(self, i):
        fid = self.frame_id(i)
        if fid not in self._calibs:
            self._calibs[fid] = Calibration(self.split_dir / "calib" / ("%s.txt" % fid))
        return self._calibs[fid]

    def lidar_path(self, i):
        return self.split_dir / "velodyne" / ("%s.bin" % self.frame_id(i))

    def scene(self, i):
        info = self.infos[i]
        fid, calib = self.frame_id(i), self.calib(i)
        d = {"frame_id": fid, "calib": calib}
        if "annos" in info:
            annos = drop_info_with_name(copy.deepcopy(info["annos"]), name="DontCare")
            cam = np.concatenate([annos["location"], annos["dimensions"], annos["rotation_y"][..., np.newaxis]], axis=1).astype(np.float32)
            d["gt_names"], d["gt_boxes"] = annos["name"], boxes3d_kitti_camera_to_lidar(cam, calib)
            plane = read_road_plane(self.split_dir / "planes" / ("%s.txt" % fid))
            if plane is not None:
                d["road_plane"] = plane
        else:        # the reference's placeholders for a frame without labels
            d["gt_names"], d["gt_boxes"] = np.array([1], np.int32), np.zeros([1, 7], np.float32)
        d["image_shape"] = copy.deepcopy(self.image_shape(i))
        return d

    def fov_crop_host(self, i):
        """the scan of frame i as the reference's __getitem__ leaves it: lidar_to_rect -> get_fov_flag -> index, on the host"""
        points = np.fromfile(str(self.lidar_path(i)), dtype=np.float32).reshape(-1, self.NUM_POINT_FEATURES)
        if not self.fov_points_only:
            return points
        calib = self.calib(i)
        return points[get_fov_flag(calib.lidar_to_rect(points[:, 0:3]), self.image_shape(i), calib)]

    # ---------------------------------------------------------------------------------------------------------------- for the evaluator
    def _indices(self, indices):
        return range(len(self)) if indices is None else indices

    def gt_annos(self, indices=None):
        return [copy.deepcopy(self.infos[i]["annos"]) for i in self._indices(indices)]

    def calibs(self, indices=None):
        return [self.calib(i) for i in self._indices(indices)]

    def image_shapes(self, indices=None):
        return [self.image_shape(i) for i in self._indices(indices)]

    def frame_ids(self, indices=None):
        return [self.frame_id(i) for i in self._indices(indices)]

    # ------------------------------------------------------------------------------------------------------------------------ batches
    def calib_blocks(self, indices):
        """(B, 32) float32: calib_block of every frame"""
        return np.stack([calib_block(self.calib(i), self.image_shape(i)) for i in indices]) if len(indices) else np.zeros((0, CALIB_FLOATS), np.float32)

    def load_batch(self, indices, device, crop=True):
        """the scans of `indices` as one resident batch.  Every .bin is read into its slice of ONE pinned buffer, which goes up in one
        copy, as do the (B, 32) calibration blocks and the offsets; btc_fov_crop then drops the rows outside the camera's view
        (crop=False, or fov_points_only=False, returns the raw rows).  One (B+1)-int read-back sizes the result, the same one
        DataProcessor.mask_and_shuffle_batch makes: DeviceAugmentor.apply and forward_raw_batch size their work from points.shape[0].
        -> {"points" (sum n', 4) f32, "scene_offsets" (B+1) device i32, "scene_counts" host list, "raw_rows" host list}"""
        import torch
        indices = list(indices)
        B, F = len(indices), self.NUM_POINT_FEATURES
        if B < 1:
            raise ValueError("load_batch: no frame")
        paths = [self.lidar_path(i) for i in indices]
        row_bytes = 4 * F
        sizes = [os.path.getsize(p) for p in paths]
        for p, s in zip(paths, sizes):
            if s % row_bytes:
                raise ValueError("%s: %d bytes is no whole number of %d-float rows" % (p, s, F))
        rows = [s // row_bytes for s in sizes]
        bounds = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
        n = int(bounds[-1])
        if n >= 2 ** 31:
            raise ValueError("load_batch: %d rows do not fit 31 bits" % n)
        # one pinned staging buffer: [points | calibration blocks | offsets], every part 16-byte aligned
        pts_bytes = n * row_bytes
        cal_at = (pts_bytes + 15) // 16 * 16
        off_at = cal_at + B * CALIB_FLOATS * 4
        stage = torch.empty((off_at + (B + 1) * 4,), dtype=torch.uint8, pin_memory=True)
        host = stage.numpy()
        for p, b0, b1 in zip(paths, bounds[:-1] * row_bytes, bounds[1:] * row_bytes):
            with open(p, "rb") as f:
                got = f.readinto(memoryview(host[b0:b1]))
            if got != b1 - b0:
                raise IOError("%s: read %d of %d bytes" % (p, got, b1 - b0))
        do_crop = bool(crop) and self.fov_points_only
        if do_crop:
            host[cal_at:off_at].view(np.float32)[:] = self.calib_blocks(indices).reshape(-1)
        host[off_at:].view(np.int32)[:] = bounds.astype(np.int32)
        dev_stage = stage.to(device, non_blocking=True)
        points = dev_stage[:pts_bytes].view(torch.float32).view(n, F)
        offs = dev_stage[off_at:].view(torch.int32)
        if not do_crop:
            return {"points": points, "scene_offsets": offs, "scene_counts": list(rows), "raw_rows": list(rows)}
        calib = dev_stage[cal_at:off_at].view(torch.float32).view(B, CALIB_FLOATS)
        out, new_offs = fov_crop(points, offs, calib)
        kept = new_offs.tolist()
        return {"points": out[:kept[B]], "scene_offsets": new_offs, "scene_counts": [kept[b + 1] - kept[b] for b in range(B)], "raw_rows": list(rows)}
