"""btc_fov_crop (csrc/fov_crop.hip, include/btcdet_hip_frames.h) through the C ABI against the numpy restatement of the header
(kitti_frames_ref.restate_crop: one float32 operation per rounded step).  Everything is exact: rows, order, bytes, out_offsets, keep_idx.

The seeded inputs are drawn to the golden fixture's decision margin (kitti_frames_ref.sample_points), the margin at which the
restatement was shown to make the reference's own decisions; the kernel is held to the restatement bit for bit either way.  The shapes
are the smallest at which the kernel can go wrong: scenes of 0 / 1 / 255 / 256 / 257 rows (one workgroup is 256 rows), a scene boundary
inside a workgroup, an empty scene between two others, more scenes inside one workgroup than calibration blocks are staged per pass (8),
ld 3 / 4 / 5 and a base pointer off 16 bytes (the scalar path), everything / nothing kept, n == 0, and the exact case on the edges."""
import numpy as np
import pytest
import torch

import kitti_frames_ref as kr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def L():
    from btcdet_amd import _lib
    return _lib.lib()


_CAL = {}


def block(k):
    """calibration block of the fixture's frame k % 4 (different matrices and image shape per k)"""
    k %= kr.N_FRAMES
    if k not in _CAL:
        c = kr.parse_calib(kr.calib_text(kr.calib_arrays(k)))
        H, W = kr.IMAGE_SHAPES[k]
        _CAL[k] = (kr.lidar_to_rect_matrix(c["R0"], c["Tr_velo2cam"]), c["P2"], W, H)
    M, P2, W, H = _CAL[k]
    return kr.calib_block(M, P2, W, H)


def scene(seed, n, k, ld=4, only=None):
    """n seeded rows for calibration k; only=True / False: rows the restatement keeps / drops only"""
    block(k)
    M, P2, W, H = _CAL[k % kr.N_FRAMES]
    rng = np.random.default_rng(seed)
    if only is None:
        return kr.sample_points(rng, n, M, P2, W, H, ld=ld)
    got = np.zeros((0, ld), np.float32)
    while got.shape[0] < n:
        p = kr.sample_points(rng, 4 * n + 64, M, P2, W, H, ld=ld)
        got = np.concatenate([got, p[kr.restate_keep(p, block(k)) == only]])
    return got[:n]


def run(pts, offsets, blocks, misalign=False, want_idx=True):
    """-> (out [:n'], out_offsets, keep_idx [:n'], the untrimmed out and keep_idx) as numpy"""
    from btcdet_amd._lib import check, stream_ptr
    n, ld = pts.shape
    B = len(offsets) - 1
    flat = torch.zeros((n * ld + 8,), dtype=torch.float32, device=DEV)
    shift = 1 if misalign else 0                                   # 4 bytes off a 16-byte boundary
    flat[shift:shift + n * ld] = torch.from_numpy(pts.reshape(-1)).to(DEV)
    src = flat[shift:shift + n * ld]
    oflat = torch.full((n * ld + 8,), -7.5, dtype=torch.float32, device=DEV)
    out = oflat[shift:shift + n * ld]
    assert (src.data_ptr() % 16 != 0) == misalign or n == 0
    offs = torch.tensor(np.asarray(offsets, np.int32), device=DEV)
    cal = torch.from_numpy(np.stack(blocks)).to(DEV)
    new_offs = torch.full((B + 1,), -9, dtype=torch.int32, device=DEV)
    idx = torch.full((max(n, 1),), -9, dtype=torch.int32, device=DEV) if want_idx else None
    ws_bytes = L().btc_fov_crop_ws_bytes(n, B)
    ws = torch.empty((max(ws_bytes, 256),), dtype=torch.uint8, device=DEV)
    check(L().btc_fov_crop(src.data_ptr(), n, ld, offs.data_ptr(), B, cal.data_ptr(), n, out.data_ptr(), new_offs.data_ptr(),
                           idx.data_ptr() if want_idx else None, ws.data_ptr(), ws_bytes, stream_ptr()), "btc_fov_crop")
    torch.cuda.synchronize()
    bounds = new_offs.cpu().numpy()
    full = out.cpu().numpy().reshape(n, ld)
    full_idx = idx.cpu().numpy() if want_idx else None
    return full[:bounds[B]], bounds, (full_idx[:bounds[B]] if want_idx else None), full, full_idx


def check_case(pts, offsets, blocks, **kw):
    want, want_offs, want_idx = kr.restate_crop(pts, offsets, blocks)
    got, bounds, idx, full, full_idx = run(pts, offsets, blocks, **kw)
    print("rows", [int(offsets[b + 1] - offsets[b]) for b in range(len(offsets) - 1)], "ld", pts.shape[1], "kept", np.diff(want_offs).tolist(), kw)
    assert bounds.tolist() == want_offs.tolist()
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    if idx is not None:
        assert idx.tolist() == want_idx.tolist()
        assert (full_idx[bounds[-1]:] == -9).all(), "keep_idx written past n'"
    assert (full[bounds[-1]:] == np.float32(-7.5)).all(), "out written past n'"
    return want_offs


def batch(sizes, ld=4, seed=0, only=None):
    pts = [scene(1000 * seed + 10 * b + ld, s, b + seed, ld, only) for b, s in enumerate(sizes)]
    return np.concatenate(pts).reshape(-1, ld), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), [block(b + seed) for b in range(len(sizes))]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_one_scene_around_a_workgroup(n):
    check_case(*batch([n], seed=n % 4))


@pytest.mark.parametrize("sizes", [(100, 200), (300, 0, 41), (257, 1, 600), (0, 513, 0), (0, 0)], ids=lambda s: "-".join(map(str, s)))
def test_scenes_with_their_own_calibration(sizes):
    """a boundary inside a workgroup, an empty scene between two others, batch 3 with a different calibration and image shape per scene"""
    pts, offs, blocks = batch(sizes)
    assert len({b.tobytes() for b in blocks}) == min(len(sizes), kr.N_FRAMES)
    want_offs = check_case(pts, offs, blocks)
    if sum(sizes) > 300:
        assert all(0 < k < s for k, s in zip(np.diff(want_offs), sizes) if s > 40), "each scene keeps some rows and drops some"


def test_more_scenes_in_a_workgroup_than_blocks_per_pass():
    sizes = [20] * 11 + [0, 3, 60, 1, 300]          # 11 scenes in the first 256 rows: two staging passes
    check_case(*batch(sizes, seed=2))


@pytest.mark.parametrize("only", [True, False], ids=["all-kept", "none-kept"])
def test_everything_and_nothing_kept(only):
    pts, offs, blocks = batch((257, 130), only=only)
    want_offs = check_case(pts, offs, blocks)
    assert want_offs.tolist() == ([0, 257, 387] if only else [0, 0, 0])


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "off16"])
@pytest.mark.parametrize("ld", [3, 4, 5])
def test_row_lengths_and_an_unaligned_base(ld, misalign):
    pts, offs, blocks = batch((257, 70, 300), ld=ld, seed=1)
    check_case(pts, offs, blocks, misalign=misalign)
    check_case(pts, offs, blocks, misalign=misalign, want_idx=False)


def test_vector_and_scalar_paths_agree_on_bits_that_are_no_numbers():
    """all ld columns are copied bit for bit: a NaN payload and a negative zero in column 3 survive both paths"""
    pts, offs, blocks = batch((300,), only=True)
    pts.view(np.uint32)[::3, 3] = 0x7FC12345
    pts.view(np.uint32)[1::3, 3] = 0x80000000
    a = run(pts, offs, blocks)[0]
    b = run(pts, offs, blocks, misalign=True)[0]
    assert a.tobytes() == b.tobytes() == pts.tobytes()


def test_exact_case_on_the_edges():
    cal, shape, pts, expect = kr.exact_case()
    blk = kr.calib_block(kr.lidar_to_rect_matrix(cal["R0"], cal["Tr_velo2cam"]), cal["P2"], shape[1], shape[0])
    assert np.array_equal(kr.gold()["exact_keep"], expect)
    for misalign in (False, True):
        got, bounds, idx, _, _ = run(pts, [0, len(pts)], [blk], misalign=misalign)
        assert idx.tolist() == np.flatnonzero(expect).tolist() and bounds.tolist() == [0, int(expect.sum())]
        assert got.tobytes() == pts[expect].tobytes()
    # the same rows as the second of two scenes, behind a scene with a camera calibration
    a, offs, blocks = batch((100,))
    both = np.concatenate([a, pts])
    check_case(both, [0, 100, 100 + len(pts)], [blocks[0], blk])


def test_the_fixture_frames_give_the_reference_rows():
    """the golden frames as one batch: the kernel keeps exactly the rows the reference's own __getitem__ kept"""
    g = kr.gold()
    pts = [g["f%d_points" % k] for k in range(kr.N_FRAMES)]
    offs = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])]).astype(np.int32)
    got, bounds, _, _, _ = run(np.concatenate(pts), offs, [block(k) for k in range(kr.N_FRAMES)])
    for k in range(kr.N_FRAMES):
        assert got[bounds[k]:bounds[k + 1]].tobytes() == g["f%d_ref_points" % k].tobytes(), k
