"""tests/roi_pool_ref.py without a GPU: its float64 formulas against conv_head.trilinear_readout and torch autograd (1e-12), its fp32
emulations of csrc/roi_pool.hip inside the derived bounds over the shared case lists, the cap on the points the float64 comparison
may leave out, and ten seeded defects of the emulations -- each has to fail some case of the lists tests/test_hip_roi_pool_edges.py
runs on the GPU, in the stage the defect belongs to."""
import numpy as np
import pytest
import torch

import roi_pool_ref as R


class _Volume:
    """what trilinear_readout asks of a sparse tensor, on CPU float64 tensors"""

    def __init__(self, feats, cells, dhw, B):
        self.features, self.cells, self.spatial_shape, self.batch_size = feats, cells, list(dhw), B

    def dense(self):
        D, H, W = self.spatial_shape
        vol = torch.zeros((self.batch_size, D, H, W, self.features.shape[1]), dtype=self.features.dtype)
        c = self.cells
        vol = vol.index_put((c[:, 0], c[:, 1], c[:, 2], c[:, 3]), self.features)
        return vol.permute(0, 4, 1, 2, 3)


def _pin_case(C=5):
    c = dict(geom="skew", dhw=(3, 7, 9), B=2, occ="checkerboard", live="null", Q=256)
    d = R.make_corners(c)
    rng = np.random.default_rng(11)
    feats = rng.standard_normal((d["n_rows"], C))
    feats[::4] = 0.0                                            # all-zero rows: read, but keep no point alive
    cells = np.argwhere(d["cell_row"] >= 0)
    order = d["cell_row"][d["cell_row"] >= 0]
    cells_by_row = np.empty_like(cells)
    cells_by_row[order] = cells
    live = (feats != 0).any(axis=1).astype(np.uint8)
    return d, feats, cells_by_row, live


def test_float64_formulas_equal_trilinear_readout_and_autograd():
    from btcdet_amd import conv_head
    d, feats, cells, live = _pin_case()
    r = R.corners_f64(d["xyz"], d["per_batch"], d["g"], d["dhw"], d["B"], d["cell_row"], live)
    Q = d["xyz"].shape[0]
    assert d["B"] * d["per_batch"] >= Q                          # no point past the batch: the dense formulation cannot index those
    tf = torch.from_numpy(feats).requires_grad_(True)
    vol = _Volume(tf, torch.from_numpy(cells), d["dhw"], d["B"])
    b = torch.from_numpy(np.arange(Q) // d["per_batch"])
    out = conv_head.trilinear_readout(vol, b, torch.from_numpy(r["f"]))      # the reference's own (z, y, x): no division enters
    ref, _ = R.gather_f64(feats, r["rows"], r["wts"])
    scale = float(np.abs(ref).max())
    assert scale > 0.1 and float(np.abs(out.detach().numpy() - ref).max()) <= 1e-12 * scale
    keep = (out.detach().abs() > 0).any(dim=-1).numpy()
    assert np.array_equal(keep.astype(np.uint8), r["flag"]) and 0 < keep.sum() < Q
    # the adjoint over the kept points, pairs sorted as _TrilinearRead.backward sorts them
    kept = np.flatnonzero(keep)
    gsel = np.random.default_rng(12).standard_normal((kept.size, feats.shape[1]))
    (g_ref,) = torch.autograd.grad(out[torch.from_numpy(kept)], tf, torch.from_numpy(gsel))
    rows_k, w_k = r["rows"][kept], r["wts"][kept]
    n_rows = feats.shape[0]
    key = np.where((rows_k >= 0) & (w_k != 0), rows_k, n_rows).reshape(-1)
    perm = np.argsort(key, kind="stable")
    seg = np.searchsorted(key[perm], np.arange(n_rows + 1))
    got, _ = R.scatter_f64(gsel, perm, seg, w_k, n_rows)
    gscale = float(g_ref.abs().max())
    assert gscale > 0.1 and float(np.abs(got - g_ref.numpy()).max()) <= 1e-12 * gscale


def _emulate_corners(W, c, defect=None):
    d = R.make_corners(c)
    rows, wts, flag = R.corners_f32(d["xyz"], d["per_batch"], d["g"], d["dhw"], d["B"], d["cell_row"], d["row_live"], defect)
    R.check_corners(W, d, rows, wts, flag, R.case_name(c))


def _emulate_scatter(W, c, defect=None):
    d = R.make_scatter(c)
    R.check_scatter(W, d, R.scatter_emu(d["grad_out"], d["pair"], d["seg"], d["wts"], d["n_rows"], defect=defect), R.scatter_name(c))


def test_emulations_sit_inside_their_bounds_and_the_cap_holds(capsys):
    W = R.Worst()
    clouds = 0
    for c in R.corner_cases():
        _emulate_corners(W, c)
        clouds += c["Q"] is not None and c["Q"] >= 255
    for c in R.gather_cases():
        d = R.make_gather(c)
        R.check_gather(W, d, R.gather_f32(d["feat"], d["rows"], d["wts"]), str(c))
    for c in R.scatter_cases():
        _emulate_scatter(W, c)
    assert clouds >= 2 * 4 * 4 * 4 and 0.0 < W.undecided <= R.CAP and 0.0 < W.coord_err < 1e-4
    assert all(r <= 1.0 for r in W.worst.values()) and set(W.worst) == set(R.STAGES)
    with capsys.disabled():
        print("\n" + W.report())


def test_exact_geometry_covers_the_grid_faces_and_integer_coordinates():
    d = R.make_corners(dict(geom="exact", dhw=(2, 3, 4), B=2, occ="full", live="null", Q=None))
    r = R.corners_f64(d["xyz"], d["per_batch"], d["g"], d["dhw"], d["B"], d["cell_row"], None)
    f = r["f"][:d["per_batch"]]
    assert r["decided"].all() and np.array_equal(R.wide(R.coords_f32(d["xyz"], d["g"])), r["f"])
    for a, n in enumerate(d["dhw"]):
        vals = set(f[:, a].tolist())
        assert {-2.0, -1.0, -0.25, 0.0, n - 1.0, n - 0.75, float(n)} <= vals, (a, sorted(vals))
    assert np.abs(f).max() > 1e5 and d["xyz"].shape[0] == d["B"] * d["per_batch"] + R.TRAILING
    assert (r["wts"] == 0).any() and ((r["rows"] >= 0) & (r["wts"] == 0)).any()          # present corners of weight zero


def test_case_lists_reach_the_unroll_and_tile_edges():
    for C in R.SCATTER_WAYS_C:
        ways = R.ways_of(C)
        L = R.scatter_lengths(ways)
        assert ways in (2, 4, 8) and {0, 1, ways, 4 * ways - 1, 4 * ways, 4 * ways + 1, 300} <= set(L)
    assert all(R.ways_of(C) is None for C in R.SCATTER_ANY_C)
    assert any(c["C"] > 64 and c["C"] % 64 for c in R.gather_cases())
    kinds = {(c["C"], R.GATHER_KINDS[(p + c["first"]) % 3]) for c in R.gather_cases() for p in range(c["M"])}
    assert all((C, k) in kinds for C in R.GATHER_C for k in R.GATHER_KINDS)
    d = R.make_scatter(R.scatter_cases()[0])
    assert np.isnan(d["wts"].reshape(-1)[d["pair"][d["seg"][-1]:]]).all() and d["pair"].size == d["seg"][-1] + R.SCATTER_TAIL


@pytest.mark.parametrize("defect", R.CORNER_DEFECTS)
def test_a_seeded_corner_defect_fails_the_corner_stage(defect):
    caught = set()
    for c in R.corner_cases():
        if c["Q"] in (None, 257):
            W = R.Worst(strict=False)
            _emulate_corners(W, c, defect)
            caught |= {s for s, r in W.worst.items() if r > 1.0}
    assert "corners_bits" in caught, caught                               # the emulation the GPU is held to bit for bit notices
    assert caught & {"corners_rows", "corners_flag", "corners_wts"}, caught  # and so does the independent float64 reference


@pytest.mark.parametrize("defect", R.SCATTER_DEFECTS)
def test_a_seeded_scatter_defect_fails_the_scatter_stage(defect):
    caught = {}
    for c in R.scatter_cases():
        W = R.Worst(strict=False)
        _emulate_scatter(W, c, defect)
        for s, r in W.worst.items():
            if r > 1.0:
                caught.setdefault(s, []).append(c["C"])
    assert set(caught) == {"scatter_bits", "scatter"}, caught
    for C in R.SCATTER_WAYS_C:                                            # every unrolled instance on its own
        assert C in caught["scatter"] and C in caught["scatter_bits"], (C, caught)
