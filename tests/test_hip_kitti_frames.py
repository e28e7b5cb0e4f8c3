"""KittiFrames.load_batch (btcdet_amd/kitti_frames.py) over the synthetic KITTI directory of tests/golden/kitti_frames.npz, rebuilt under
tmp_path: the resident, device-cropped batch holds, per scene and byte for byte, the points the reference's own
KittiDataset.__getitem__ handed to prepare_data (FOV_POINTS_ONLY), as one batch of all frames and as batches of one; crop=False returns
the raw rows; and the result goes through DataProcessor.forward_raw_batch to the voxel keys of the host-cropped upload (exact by
construction: the same rows in the same order)."""
import numpy as np
import pytest
import torch

import kitti_frames_ref as kr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    from btcdet_amd.kitti_frames import KittiFrames
    return KittiFrames(kr.build_dir(kr.gold(), tmp_path_factory.mktemp("kitti")), "train")


def _check(batch, ks):
    g = kr.gold()
    want = [g["f%d_ref_points" % k] for k in ks]
    assert batch["scene_counts"] == [w.shape[0] for w in want]
    assert batch["raw_rows"] == [g["f%d_points" % k].shape[0] for k in ks]
    offs = batch["scene_offsets"]
    assert offs.dtype == torch.int32 and offs.is_cuda and offs.cpu().tolist() == np.concatenate([[0], np.cumsum(batch["scene_counts"])]).tolist()
    pts = batch["points"]
    assert pts.is_cuda and pts.dtype == torch.float32 and pts.shape == (sum(batch["scene_counts"]), 4) and pts.is_contiguous()
    host, bounds = pts.cpu().numpy(), offs.cpu().tolist()
    for b, w in enumerate(want):
        assert host[bounds[b]:bounds[b + 1]].tobytes() == w.tobytes(), ("scene", b, "frame", ks[b])


def test_load_batch_gives_the_reference_points(frames):
    _check(frames.load_batch(range(kr.N_FRAMES), DEV), list(range(kr.N_FRAMES)))
    _check(frames.load_batch([2, 0], DEV), [2, 0])
    for k in range(kr.N_FRAMES):                 # batches of one, the frame whose single row is dropped included
        _check(frames.load_batch([k], DEV), [k])


def test_crop_false_returns_the_raw_rows(frames):
    from btcdet_amd.kitti_frames import KittiFrames
    g = kr.gold()
    raw = np.concatenate([g["f%d_points" % k] for k in range(kr.N_FRAMES)])
    for fr, kw in ((frames, dict(crop=False)), (KittiFrames(frames.root, "train", fov_points_only=False), {})):
        b = fr.load_batch(range(kr.N_FRAMES), DEV, **kw)
        assert b["points"].cpu().numpy().tobytes() == raw.tobytes()
        assert b["scene_counts"] == b["raw_rows"] == kr.N_POINTS
        assert b["scene_offsets"].dtype == torch.int32 and b["scene_offsets"].cpu().tolist() == np.concatenate([[0], np.cumsum(kr.N_POINTS)]).tolist()
    with pytest.raises(ValueError):
        frames.load_batch([], DEV)


def test_the_batch_goes_through_forward_raw_batch(frames):
    """load_batch -> forward_raw_batch gives the six voxel tensors of the host-cropped upload, with the same shuffle_idx"""
    from btcdet_amd.config import load_cfg
    from btcdet_amd.processor import DataProcessor
    d = load_cfg().DATA_CONFIG
    proc = DataProcessor(d.DATA_PROCESSOR, point_cloud_range=np.array(d.OCC.POINT_CLOUD_RANGE, dtype=np.float32), training=True, occ_config=d.OCC,
                         det_point_cloud_range=np.array(d.POINT_CLOUD_RANGE, dtype=np.float32))
    ks = [0, 1, 2]
    host = [frames.fov_crop_host(k) for k in ks]
    h_pts = torch.from_numpy(np.concatenate(host)).to(DEV)
    h_offs = torch.from_numpy(np.cumsum([0] + [h.shape[0] for h in host]).astype(np.int32)).to(DEV)
    rot = torch.tensor([0.0, 10.0, -5.0], dtype=torch.float32, device=DEV)
    flag = getattr(proc, "_shuffle_flag", None)      # the permutations need the masked counts: one masking pass without the shuffle tells them
    proc._shuffle_flag = False
    _, _, _, counts = proc.mask_and_shuffle_batch(h_pts, None, h_offs)
    proc._shuffle_flag = flag
    perms = [np.random.default_rng(5 + b).permutation(c) for b, c in enumerate(counts)] if proc._shuffle_enabled() else None
    ref = proc.forward_raw_batch(h_pts, None, h_offs, rot, shuffle_idx=perms)
    batch = frames.load_batch(ks, DEV)
    got = proc.forward_raw_batch(batch["points"], None, batch["scene_offsets"], rot, shuffle_idx=perms)
    assert got["scene_counts"] == ref["scene_counts"] == counts and min(counts) > 0
    for k in ("voxels", "voxel_coords", "voxel_num_points", "det_voxels", "det_voxel_coords", "det_voxel_num_points"):
        assert got[k].shape == ref[k].shape and got[k].shape[0] > 0, k
        assert torch.equal(got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k],
                           ref[k].view(torch.int32) if ref[k].dtype == torch.float32 else ref[k]), k
