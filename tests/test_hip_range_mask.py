"""btc_range_mask_compact (csrc/prestep.hip, include/btcdet_hip.h) through the C ABI against numpy: per scene
keep = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1), points[keep], pre[keep], cumsum for the offsets, flatnonzero for keep_idx.
The kernel only compares and copies, so everything is exact: rows, order, bytes, out_offsets, keep_idx; every output is pre-filled
with a sentinel that the rows past n' must still hold.

The shapes are the smallest at which the compaction can go wrong: one scene of 0 / 1 / 63 / 64 / 65 / 255 / 256 / 257 / 513 rows (a wave
is 64 rows, a workgroup 256), a scene boundary inside a wave, inside a workgroup and exactly on a multiple of 256, empty scenes first /
middle / last, everything / nothing kept, rows exactly on the four limits and one float32 ulp outside them, NaN coordinates, payload bits
that are no numbers, ld 2 / 3 / 4 / 5 with a second array of ld_b 3 / 4 or none, with and without keep_idx, and each of the four bases in
turn 4 bytes off a 16-byte boundary (the scalar path), and one scene of 256 * 2048 + 257 rows (more workgroup counts than one tile of
the device scan)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIM = np.array([0.0, -40.0, 70.4, 40.0], np.float32)          # x_lo, y_lo, x_hi, y_hi
FILL, IFILL = np.float32(-7.5), -9
ARRAYS = ("points", "out", "points_b", "out_b")


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def keep_mask(pts, offsets, lim=LIM):
    keep = np.zeros(pts.shape[0], bool)
    for b in range(len(offsets) - 1):
        p = pts[offsets[b]:offsets[b + 1]]
        with np.errstate(invalid="ignore"):
            keep[offsets[b]:offsets[b + 1]] = (p[:, 0] >= lim[0]) & (p[:, 0] <= lim[2]) & (p[:, 1] >= lim[1]) & (p[:, 1] <= lim[3])
    return keep


def expect(pts, offsets, pre, lim=LIM):
    """-> (points[keep], pre[keep] or None, out_offsets, keep_idx)"""
    keep = keep_mask(pts, offsets, lim)
    per_scene = [int(keep[offsets[b]:offsets[b + 1]].sum()) for b in range(len(offsets) - 1)]
    return pts[keep], (pre[keep] if pre is not None else None), np.concatenate([[0], np.cumsum(per_scene)]).astype(np.int32), np.flatnonzero(keep)


def batch(sizes, ld=4, ld_b=4, seed=0, only=None):
    """seeded rows, about 4 in 10 inside LIM (only=True / False: all / none inside); -> (points, offsets, pre or None)"""
    rng = np.random.default_rng(100 * seed + 10 * ld + (ld_b or 0))
    n = int(sum(sizes))
    pts = rng.uniform(-50.0, 50.0, (n, ld)).astype(np.float32)
    if only is None:
        pts[:, 0] = rng.uniform(-35.0, 105.0, n)
        pts[:, 1] = rng.uniform(-60.0, 60.0, n)
    else:
        pts[:, 0] = rng.uniform(1.0, 70.0, n) if only else rng.uniform(71.0, 90.0, n)
        pts[:, 1] = rng.uniform(-39.0, 39.0, n)
    pre = rng.uniform(-50.0, 50.0, (n, ld_b)).astype(np.float32) if ld_b else None
    return pts, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), pre


def placed(a, off16, fill=None):
    """a device buffer for rows shaped like `a` whose base is 16-byte aligned, or 4 bytes past such a boundary; holds `a`, or `fill`"""
    flat = torch.zeros((a.size + 8,), dtype=torch.float32, device=DEV)
    view = flat[1:1 + a.size] if off16 else flat[:a.size]
    if fill is None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    else:
        view.fill_(float(fill))
    assert (view.data_ptr() % 16 != 0) == bool(off16) or a.size == 0
    return view


def run(pts, offsets, pre=None, lim=LIM, off16=(), want_idx=True):
    """-> (out, out_b or None, out_offsets, keep_idx or None), untrimmed, as numpy; off16: names of ARRAYS whose base is 4 bytes off"""
    from btcdet_amd._lib import check, f32p, stream_ptr
    n, ld = pts.shape
    B = len(offsets) - 1
    src = placed(pts, "points" in off16)
    out = placed(pts, "out" in off16, FILL)
    src_b = out_b = None
    ld_b = 0
    if pre is not None:
        ld_b = pre.shape[1]
        src_b = placed(pre, "points_b" in off16)
        out_b = placed(pre, "out_b" in off16, FILL)
    offs = torch.tensor(np.asarray(offsets, np.int32), device=DEV)
    new_offs = torch.full((B + 1,), IFILL, dtype=torch.int32, device=DEV)
    idx = torch.full((max(n, 1),), IFILL, dtype=torch.int32, device=DEV) if want_idx else None
    ws_bytes = L().btc_range_mask_ws_bytes(n)
    ws = torch.full((max(ws_bytes, 256),), 0xA5, dtype=torch.uint8, device=DEV)
    h_lim = np.ascontiguousarray(lim, dtype=np.float32)
    check(L().btc_range_mask_compact(src.data_ptr(), src_b.data_ptr() if pre is not None else None, n, ld, ld_b, offs.data_ptr(), B,
                                     f32p(h_lim), out.data_ptr(),
                                     out_b.data_ptr() if pre is not None else None, new_offs.data_ptr(),
                                     idx.data_ptr() if want_idx else None, ws.data_ptr(), ws_bytes, stream_ptr()), "btc_range_mask_compact")
    torch.cuda.synchronize()
    return (out.cpu().numpy().reshape(n, ld), out_b.cpu().numpy().reshape(n, ld_b) if pre is not None else None, new_offs.cpu().numpy(),
            idx.cpu().numpy() if want_idx else None)


def check_case(pts, offsets, pre=None, lim=LIM, **kw):
    want, want_b, want_offs, want_idx = expect(pts, offsets, pre, lim)
    out, out_b, bounds, idx = run(pts, offsets, pre, lim, **kw)
    print("rows", np.diff(offsets).tolist(), "ld", pts.shape[1], "ld_b", None if pre is None else pre.shape[1], "kept", np.diff(want_offs).tolist(), kw)
    assert bounds.tolist() == want_offs.tolist()
    k = int(want_offs[-1])
    assert out[:k].tobytes() == want.tobytes()
    assert (out[k:] == FILL).all(), "out written past n'"
    if pre is not None:
        assert out_b[:k].tobytes() == want_b.tobytes()
        assert (out_b[k:] == FILL).all(), "out_b written past n'"
    if idx is not None:
        assert idx[:k].tolist() == want_idx.tolist()
        assert (idx[k:] == IFILL).all(), "keep_idx written past n'"
    return want_offs


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 513])
def test_one_scene_at_wave_and_workgroup_edges(n):
    want_offs = check_case(*batch([n], seed=n))
    assert n < 63 or 0 < want_offs[-1] < n, "some rows kept, some dropped"


def test_more_workgroup_counts_than_one_scan_tile():
    """256 * 2048 + 257 rows are 2050 workgroups of the count stage and the device scan takes 2048 counts per workgroup: two scan
    workgroups, the second of which starts from the sum of the first's counts"""
    n = 256 * 2048 + 257
    pts, offs, _ = batch([n], ld_b=None, seed=11)
    want_offs = check_case(pts, offs)
    assert want_offs[-1] > keep_mask(pts[:256 * 2048], [0, 256 * 2048]).sum() > 0, "rows are kept in both scan tiles"


@pytest.mark.parametrize("sizes", [(100, 200), (300, 0, 41), (257, 1, 600), (0, 513, 0), (0, 0), (256, 256, 1)], ids=lambda s: "-".join(map(str, s)))
def test_scene_boundaries(sizes):
    """a boundary inside a wave and inside a workgroup, empty scenes first / middle / last, a boundary exactly on a multiple of 256"""
    want_offs = check_case(*batch(sizes, seed=len(sizes)))
    assert all(0 < k < s for k, s in zip(np.diff(want_offs), sizes) if s > 40), "each scene keeps some rows and drops some"


@pytest.mark.parametrize("only", [True, False], ids=["all-kept", "none-kept"])
def test_everything_and_nothing_kept(only):
    want_offs = check_case(*batch((257, 130), only=only))
    assert want_offs.tolist() == ([0, 257, 387] if only else [0, 0, 0])


def edge_rows():
    """rows exactly on each limit and on two corners (kept), rows one float32 ulp outside each limit (dropped), x or y NaN (dropped)"""
    x0, y0, x1, y1 = LIM
    xm, ym = np.float32(30.0), np.float32(1.0)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    on = [(x0, ym), (x1, ym), (xm, y0), (xm, y1), (x0, y0), (x1, y1)]
    off = [(np.nextafter(x0, -inf), ym), (np.nextafter(x1, inf), ym), (xm, np.nextafter(y0, -inf)), (xm, np.nextafter(y1, inf)), (nan, ym), (xm, nan),
           (nan, nan)]
    pts = np.zeros((len(on) + len(off), 4), np.float32)
    pts[:, :2] = np.array(on + off, np.float32)
    pts[:, 2] = np.arange(len(pts))
    order = np.random.default_rng(5).permutation(len(pts))
    return pts[order], (order < len(on))


@pytest.mark.parametrize("off16", [(), ("points",)], ids=["vector", "scalar"])
def test_limits_are_inclusive_and_a_nan_drops_the_row(off16):
    rows, kept = edge_rows()
    filler, _, _ = batch((250,), seed=7)
    pts = np.concatenate([filler[:60], rows, filler[60:237], rows])       # the edge rows across a wave edge (64) and a workgroup edge (256)
    want = np.concatenate([keep_mask(filler[:60], [0, 60]), kept, keep_mask(filler[60:237], [0, 177]), kept])
    offsets = np.array([0, 66, len(pts)], np.int32)
    assert keep_mask(pts, offsets).tolist() == want.tolist()
    pre = (pts[:, :3] * 2 + 1).astype(np.float32)
    check_case(pts, offsets, pre, off16=off16)
    out, _, bounds, idx = run(pts, offsets, pre, off16=off16)
    assert idx[:bounds[-1]].tolist() == np.flatnonzero(want).tolist()


def test_vector_and_scalar_paths_agree_on_bits_that_are_no_numbers():
    """all columns are copied bit for bit: a NaN payload and a negative zero in column 3 survive both paths, in both arrays"""
    pts, offs, pre = batch((300,), only=True)
    for a in (pts, pre):
        a.view(np.uint32)[::3, 3] = 0x7FC12345
        a.view(np.uint32)[1::3, 3] = 0x80000000
    a, a_b, _, _ = run(pts, offs, pre)
    for name in ARRAYS:
        b, b_b, _, _ = run(pts, offs, pre, off16=(name,))
        assert a.tobytes() == b.tobytes() == pts.tobytes(), name
        assert a_b.tobytes() == b_b.tobytes() == pre.tobytes(), name


@pytest.mark.parametrize("ld_b", [None, 3, 4])
@pytest.mark.parametrize("ld", [2, 3, 4, 5])
def test_row_lengths_with_and_without_a_second_array(ld, ld_b):
    pts, offs, pre = batch((257, 70, 300), ld=ld, ld_b=ld_b, seed=1)
    check_case(pts, offs, pre)
    check_case(pts, offs, pre, want_idx=False)


@pytest.mark.parametrize("name", ARRAYS)
def test_one_unaligned_base_takes_the_scalar_path_to_the_same_bytes(name):
    pts, offs, pre = batch((257, 70, 300), seed=2)
    check_case(pts, offs, pre, off16=(name,))
    check_case(pts, offs, pre, off16=(name,), want_idx=False)
    got, aligned = run(pts, offs, pre, off16=(name,)), run(pts, offs, pre)
    assert all(g.tobytes() == a.tobytes() for g, a in zip(got, aligned))
