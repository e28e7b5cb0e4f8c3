"""csrc/pointnet2.hip on its decision boundaries.  tests/test_hip_pointnet2.py draws continuous random coordinates, where no distance
ever equals a radius or another distance; here every scene lies on an integer / half-integer lattice, so every squared distance is
exact in fp32 and float64 alike, and the kernel, the C oracle and a brute-force numpy scan written in this file must agree bit for
bit: d2 == outer2 (strict <) and d2 == inner2 (>=) in the ball / shell query, nsample reached in the middle of a 64-lane ballot, a
first hit in the second LDS tile, scenes of 1023 / 1024 / 1025 points, empty scenes on either side; equal distances, two and three
known points and 1024 / 1025 of them in three_nn; furthest point sampling one past its two kernel-selection thresholds; the
gradients of grouping and interpolation with every query on ONE row (the worst atomic contention) against float64 within
(L + 1) u sum |terms| for L additions in an unspecified order."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def half_lattice(rng, n, span, centre=(0.0, 0.0, 0.0)):
    """n points with integer or half-integer coordinates within span of centre"""
    return (rng.integers(-2 * span, 2 * span + 1, (n, 3)) / 2.0 + np.asarray(centre)).astype(np.float32)


def scene_starts(cnt):
    return np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)


def d2_all(q, pts):
    """squared distances of one query to a scene, float64 (exact on the lattice)"""
    d = np.asarray(q, np.float64)[None, :] - np.asarray(pts, np.float64)
    return (d * d).sum(axis=1)


# ------------------------------------------------------------------------------------------------------------------ ball / shell query
def ball_query_scan(radius, nsample, xyz, cnt, new_xyz, ncnt):
    """brute force: hits in index order, padded with the first hit; an empty ball is a row of zeros and a set flag"""
    inner2, outer2 = (float(radius[0]) ** 2, float(radius[1]) ** 2) if isinstance(radius, (list, tuple)) else (-1.0, float(radius) ** 2)
    idx, empty = np.zeros((new_xyz.shape[0], nsample), np.int32), np.zeros(new_xyz.shape[0], bool)
    ps, qs = scene_starts(cnt), scene_starts(ncnt)
    on_edge = 0
    for b in range(len(cnt)):
        pts = xyz[ps[b]:ps[b] + cnt[b]]
        for q in range(qs[b], qs[b] + ncnt[b]):
            d2 = d2_all(new_xyz[q], pts)
            on_edge += int(((d2 == outer2) | (d2 == inner2)).sum())
            hits = np.flatnonzero((d2 >= inner2) & (d2 < outer2))
            if hits.size == 0:
                empty[q] = True
            else:
                idx[q] = hits[0]
                k = min(hits.size, nsample)
                idx[q, :k] = hits[:k]
    return idx, empty, on_edge


RING25 = [(3, 4, 0), (0, 0, 5), (-3, -4, 0), (5, 0, 0), (0, 4, 3), (0, -5, 0)]       # d2 == 25 from the origin
INSIDE25 = [(0, 0, 4.5), (3, 3.5, 0), (2, 2, 2), (1, 1, 1), (-4.5, 0, 1.5), (0.5, 0.5, 0.5)]


def _boundary_scene(rng, centre, extra, span=6):
    pts = np.concatenate([np.array(RING25 + INSIDE25, np.float32) + np.asarray(centre, np.float32), half_lattice(rng, extra, span, centre)])
    return pts[rng.permutation(pts.shape[0])]


def ball_cases():
    rng = np.random.default_rng(17)
    out = {}
    # radius 5: offsets (3, 4, 0) and (0, 0, 5) have d2 == 25 and are excluded
    xyz = _boundary_scene(rng, (10, 10, 10), 200)
    new = np.concatenate([[[10, 10, 10]], half_lattice(rng, 20, 3, (10, 10, 10)), [[100, 100, 100]]]).astype(np.float32)   # the last: an empty ball
    for ns in (16, 1):
        out[f"ball_r5_nsample{ns}"] = dict(radius=5.0, nsample=ns, xyz=xyz, cnt=[xyz.shape[0]], new_xyz=new, ncnt=[new.shape[0]], edge=True)
    # shell [5, 13]: d2 == 25 included, d2 == 169 excluded
    ring = np.array(RING25 + [(5, 12, 0), (0, 0, 13), (0, 0, 12.5), (12, 5, 0), (0, 0, 4.5), (13, 0, 0)], np.float32)
    xyz = np.concatenate([ring, half_lattice(rng, 300, 10)])
    xyz = xyz[rng.permutation(xyz.shape[0])]
    new = np.concatenate([[[0, 0, 0]], half_lattice(rng, 20, 4)]).astype(np.float32)
    out["shell_5_13"] = dict(radius=[5.0, 13.0], nsample=32, xyz=xyz, cnt=[xyz.shape[0]], new_xyz=new, ncnt=[new.shape[0]], edge=True)
    # nsample 70 against 64 + 10 (+ 12 later) hits: the cut falls inside the second 64-lane ballot
    near = np.unique(half_lattice(rng, 4000, 2), axis=0)
    near = near[rng.permutation(near.shape[0])][:64 + 10 + 12]
    far = half_lattice(rng, 200, 3, (40, 40, 40))
    second = np.concatenate([far[:54], near[64:74]])[rng.permutation(64)]
    third = np.concatenate([far[54:106], near[74:86]])[rng.permutation(64)]
    xyz = np.concatenate([near[:64], second, third])
    new = np.array([[0, 0, 0], [0, 0, 0.5], [40, 40, 40], [0, 0, 0]], np.float32)
    out["cut_in_second_ballot"] = dict(radius=5.0, nsample=70, xyz=xyz, cnt=[192], new_xyz=new, ncnt=[4], edge=False)
    # more samples than hits: padded with the first hit, which is not point 0
    xyz = np.concatenate([far[:9], near[:2], far[9:40], near[2:5]])
    out["pad_with_first_hit"] = dict(radius=5.0, nsample=70, xyz=xyz, cnt=[xyz.shape[0]], new_xyz=new, ncnt=[4], edge=False)
    # the first hit at point 1030 of a 1100-point scene: in the second LDS tile
    xyz = half_lattice(rng, 1100, 3, (40, 40, 40))
    xyz[[1030, 1031, 1050, 1099]] = near[:4]
    out["late_first_hit"] = dict(radius=5.0, nsample=16, xyz=xyz, cnt=[1100], new_xyz=new[:3], ncnt=[3], edge=False)
    # scenes of 1023 / 1024 / 1025 points whose last point is a hit
    cnt = [1023, 1024, 1025]
    xyz = half_lattice(rng, sum(cnt), 3, (40, 40, 40))
    for s, n in zip(scene_starts(cnt), cnt):
        xyz[[s + 5, s + n - 2, s + n - 1]] = near[:3]
    new = np.concatenate([new[:3]] * 3)
    out["tile_edges"] = dict(radius=5.0, nsample=8, xyz=xyz, cnt=cnt, new_xyz=new, ncnt=[3, 3, 3], edge=False)
    # empty scenes on either side; one 16-query workgroup straddles scenes 1 and 3
    cnt = [3, 1025, 0, 64]
    xyz = _boundary_scene(rng, (0, 0, 0), sum(cnt) - len(RING25) - len(INSIDE25))
    new = np.concatenate([[[0, 0, 0]], half_lattice(rng, 24, 3)]).astype(np.float32)
    out["empty_scenes"] = dict(radius=5.0, nsample=16, xyz=xyz, cnt=cnt, new_xyz=new, ncnt=[0, 5, 0, 20], edge=True)
    return out


BALL = ball_cases()


@pytest.mark.parametrize("name", list(BALL))
def test_ball_query_on_the_lattice(name):
    from btcdet_amd import pointnet2_stack as p2
    c = BALL[name]
    cnt, ncnt = np.asarray(c["cnt"], np.int32), np.asarray(c["ncnt"], np.int32)
    assert c["xyz"].shape[0] == cnt.sum() and c["new_xyz"].shape[0] == ncnt.sum()
    bidx, bempty, on_edge = ball_query_scan(c["radius"], c["nsample"], c["xyz"], cnt, c["new_xyz"], ncnt)
    assert on_edge > 0 or not c["edge"]                                       # the case does put distances on its radii
    oidx, oempty = orc.ball_query(c["radius"], c["nsample"], c["xyz"], cnt, c["new_xyz"], ncnt)
    np.testing.assert_array_equal(oidx, bidx)
    np.testing.assert_array_equal(oempty, bempty)
    for _ in range(2):
        idx, empty = p2.ball_query(c["radius"], c["nsample"], t(c["xyz"]), t(cnt), t(c["new_xyz"]), t(ncnt))
        np.testing.assert_array_equal(idx.cpu().numpy(), bidx)
        np.testing.assert_array_equal(empty.cpu().numpy(), bempty)
    if name == "cut_in_second_ballot":
        assert bidx[0, 63] == 63 and 64 <= bidx[0, 64] and bidx[0, 69] < 128 and not bempty[0]
    if name == "late_first_hit":
        assert bidx[0, 0] == 1030 and bidx[0, 4] == 1030
    if name == "tile_edges":
        assert [int(bidx[3 * k, 2]) for k in range(3)] == [1022, 1023, 1024]


# ------------------------------------------------------------------------------------------------------------------ three_nn
def three_nn_scan(unknown, uc, known, kc):
    """brute force: the three smallest squared distances, the earliest index among equals; missing neighbours: inf, the scene's row 0"""
    dist, idx = np.full((unknown.shape[0], 3), np.inf, np.float32), np.zeros((unknown.shape[0], 3), np.int32)
    us, ks = scene_starts(uc), scene_starts(kc)
    ties = 0
    for b in range(len(uc)):
        kn = known[ks[b]:ks[b] + kc[b]]
        idx[us[b]:us[b] + uc[b]] = ks[b]
        for q in range(us[b], us[b] + uc[b]):
            d2 = d2_all(unknown[q], kn)
            order = np.argsort(d2, kind="stable")[:3]
            ties += int(np.unique(np.sort(d2)[:4]).size < min(4, d2.size))          # equal distances among the nearest four
            dist[q, :order.size] = np.sqrt(d2[order].astype(np.float32))
            idx[q, :order.size] = order + ks[b]
    return dist, idx, ties


def three_nn_cases():
    rng = np.random.default_rng(23)
    out = {}
    star = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)], np.float32)
    # equal distances everywhere (span 2, 40 known points); the scene boundary of the unknown points at 200, inside the first block
    rest = half_lattice(rng, 34, 2)
    rest[(rest * rest).sum(axis=1) <= 1.0] = 2.0                              # nothing nearer to the origin than the six of `star`
    out["equidistant"] = dict(unknown=np.concatenate([[[0, 0, 0]], half_lattice(rng, 299, 2)]).astype(np.float32), uc=[200, 100],
                              known=np.concatenate([star, rest, half_lattice(rng, 40, 2)]), kc=[40, 40], ties=True)
    out["three_and_two_known"] = dict(unknown=half_lattice(rng, 10, 2), uc=[5, 5], known=half_lattice(rng, 5, 2), kc=[3, 2], ties=False)
    known = half_lattice(rng, 2049, 3, (30, 30, 30))
    known[[1023, 1022, 7]] = star[:3]
    known[[1024 + 1024, 1024 + 1023, 1024 + 1]] = star[3:]
    unknown = half_lattice(rng, 20, 1)
    unknown[[0, 10]] = 0.0                                                    # equidistant from its scene's three, first and last tile
    out["tile_edges"] = dict(unknown=unknown, uc=[10, 10], known=known, kc=[1024, 1025], ties=True)
    return out


NN = three_nn_cases()


@pytest.mark.parametrize("name", list(NN))
def test_three_nn_on_the_lattice(name):
    from btcdet_amd import pointnet2_stack as p2
    c = NN[name]
    uc, kc = np.asarray(c["uc"], np.int32), np.asarray(c["kc"], np.int32)
    bdist, bidx, ties = three_nn_scan(c["unknown"], uc, c["known"], kc)
    assert (ties > 0) == c["ties"]
    odist, oidx = orc.three_nn(c["unknown"], uc, c["known"], kc)
    np.testing.assert_array_equal(oidx, bidx)
    np.testing.assert_array_equal(odist, bdist)
    for _ in range(2):
        dist, idx = p2.three_nn(t(c["unknown"]), t(uc), t(c["known"]), t(kc))
        np.testing.assert_array_equal(idx.cpu().numpy(), bidx)
        np.testing.assert_array_equal(dist.cpu().numpy(), bdist)
    if name == "equidistant":
        assert bidx[0].tolist() == [0, 1, 2]
    if name == "three_and_two_known":
        assert np.isinf(bdist[5:, 2]).all() and np.isfinite(bdist[:5]).all() and (bidx[5:, 2] == 3).all()


# ------------------------------------------------------------------------------------------------------------------ furthest point sampling
def fps_scan(xyz, m):
    """fp32 scan (exact on the lattice); among equal maxima the smallest (bit-reversed k mod T, k), T = the largest power of two
    <= n, at most 1024"""
    B, n, _ = xyz.shape
    T, log2T = 1, 0
    while T * 2 <= n and T < 1024:
        T, log2T = T * 2, log2T + 1
    k = np.arange(n)
    key = np.zeros(n, np.int64)
    for bit in range(log2T):
        key |= (((k & (T - 1)) >> bit) & 1) << (log2T - 1 - bit)
    out = np.zeros((B, m), np.int32)
    for b in range(B):
        p = xyz[b].astype(np.float32)
        temp = np.full(n, 1e10, np.float32)
        last = 0
        for j in range(1, m):
            d = p - p[last]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            temp = np.minimum(d2, temp)
            best = np.flatnonzero(temp == temp.max())
            last = int(best[np.lexsort((best, key[best]))[0]])
            out[b, j] = last
    return out


@pytest.mark.parametrize("lattice", [True, False], ids=["lattice", "continuous"])
@pytest.mark.parametrize("n", [4097, 16385])
def test_furthest_point_sampling_past_the_thresholds(n, lattice):
    from btcdet_amd import pointnet2_stack as p2
    rng = np.random.default_rng(n + lattice)
    xyz = (rng.integers(0, 4, (2, n, 3)) if lattice else rng.uniform(-30, 30, (2, n, 3))).astype(np.float32)
    ref = fps_scan(xyz, 8)
    np.testing.assert_array_equal(orc.furthest_point_sample(xyz, 8), ref)
    for _ in range(2):
        np.testing.assert_array_equal(p2.furthest_point_sample(t(xyz), 8).cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------------------------ gradients on one row
def _within(got, terms, where):
    """terms (L, ...) float64: got against their float64 sum within (L + 1) u sum |terms|"""
    L = terms.shape[0]
    ref, bound = terms.sum(axis=0), (L + 1) * U * np.abs(terms).sum(axis=0)
    worst = float((np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-30)).max())
    print(f"{where}: L = {L}, worst |got - ref| / bound = {worst:.3g}")
    assert np.isfinite(got).all() and worst <= 1.0, (where, worst)


@pytest.mark.parametrize("nsample", [1, 16])
@pytest.mark.parametrize("C", [1, 13])
def test_grouping_gradient_with_every_query_on_one_row(C, nsample):
    from btcdet_amd import pointnet2_stack as p2
    rng = np.random.default_rng(100 * C + nsample)
    fc, ic, row = np.array([5, 4], np.int32), np.array([0, 400], np.int32), 2
    idx = np.full((400, nsample), row, np.int32)                             # scene 1's row 2 = stacked row 7
    f = t(rng.standard_normal((9, C)).astype(np.float32)).requires_grad_(True)
    out = p2.grouping_operation(f, t(fc), t(idx), t(ic))
    assert torch.equal(out, f.detach()[5 + row].view(1, C, 1).expand(400, C, nsample))
    g = rng.standard_normal((400, C, nsample)).astype(np.float32)
    out.backward(t(g))
    got = f.grad.cpu().numpy()
    assert not got[np.arange(9) != 5 + row].any()
    _within(got[5 + row], g.astype(np.float64).transpose(0, 2, 1).reshape(-1, C), f"grouping C={C} nsample={nsample}")


@pytest.mark.parametrize("C", [1, 13])
def test_interpolation_gradient_with_every_query_on_one_row(C):
    from btcdet_amd import pointnet2_stack as p2
    rng = np.random.default_rng(200 + C)
    N, row = 2000, 3
    idx = np.full((N, 3), row, np.int32)
    w = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    f = t(rng.standard_normal((6, C)).astype(np.float32)).requires_grad_(True)
    out = p2.three_interpolate(f, t(idx), t(w))
    g = rng.standard_normal((N, C)).astype(np.float32)
    out.backward(t(g))
    got = f.grad.cpu().numpy()
    assert not got[np.arange(6) != row].any()
    terms = (g.astype(np.float64)[:, None, :] * w.astype(np.float64)[:, :, None]).reshape(-1, C)
    _within(got[row], terms, f"interpolation C={C}")
