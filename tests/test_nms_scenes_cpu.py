"""Pins the scenes of tests/nms_scenes.py, the expectation of tests/test_hip_nms_chain_edges.py: the kept list the builder states by
construction equals a plain float64 greedy loop on every scene, and the oracle's restatement of the reference's fp32 formulation
(oracle/btc_oracle.c orc_nms) reproduces it on the scenes of up to ~5000 boxes; the oracle's IoU on special geometry against the closed
forms; and what the oracle does with non-finite rows, which is what the device chains are held to."""
import numpy as np
import pytest

import nms_scenes as S
from oracle import oracle as orc

ORACLE_MAX_N = 5000
_SCENES = S.all_scenes()


def _scores(n):
    return (n - np.arange(n)).astype(np.float32)     # sorted order: position 0 is the best box


@pytest.mark.parametrize("name,thunk", _SCENES, ids=[s[0] for s in _SCENES])
def test_expected_list_is_the_float64_greedy_chain_and_the_oracle_agrees(name, thunk):
    sc = thunk()
    ref = S.reference_keep(sc.boxes, sc.rotated, ious=sc.ious)
    np.testing.assert_array_equal(sc.keep, ref)
    assert all(abs(v - S.THRESH) >= S.MARGIN for v in sc.ious.values())
    if sc.n <= ORACLE_MAX_N:
        np.testing.assert_array_equal(orc.nms(sc.boxes, _scores(sc.n), S.THRESH, rotated=sc.rotated), sc.keep)


def test_primitives_decide_as_documented():
    sc = S.build(12, pairs=[(0, 5)], triples=[(1, 2, 3), (4, 9, 7)], piles=[(6, 8, 10, 11)])
    assert sc.keep.tolist() == [0, 1, 3, 4, 6, 7]     # c = 3 kept although b = 2 overlaps it: b was itself suppressed
    v = sorted(sc.ious.values())
    np.testing.assert_allclose(v[0], 1 / 7, rtol=1e-5)
    np.testing.assert_allclose([x for x in v if 0.4 < x < 0.5], 5 / 11, rtol=1e-5)
    np.testing.assert_allclose([x for x in v if x > 0.5], 1.0, rtol=1e-5)
    assert len(v) == 1 + 2 * 3 + 6                     # the pair, three per triple, six in the pile of four: no other pair is near


@pytest.mark.parametrize("rotated", [True, False])
def test_reference_evaluates_every_overlapping_pair(rotated):
    """the near-pair shortcut of the float64 reference drops no pair that overlaps: against the full n x n loop on a small scene"""
    sc = S.build(130, pairs=[(0, 1), (3, 64), (5, 129)], triples=[(7, 9, 70), (8, 100, 20)], piles=[(10, 11, 66, 128)], rotated=rotated)
    b = sc.boxes.astype(np.float64)
    for i in range(sc.n):
        for j in range(i + 1, sc.n):
            v = S.iou_f64(b[i], b[j], rotated)
            assert v == pytest.approx(sc.ious.get((i, j), 0.0), abs=1e-12)


@pytest.mark.parametrize("m,rotated", [(1024, True), (1000, False)])
def test_removed_candidates_neither_stay_nor_suppress(m, rotated):
    """the fused chain's score threshold: the expectation with candidates removed is the float64 chain over the others"""
    sc = S.fused(m, rotated, True)
    alive = np.setdiff1d(np.arange(m), S.FUSED_REMOVED)
    ref = alive[S.reference_keep(sc.boxes[alive], rotated)]
    np.testing.assert_array_equal(sc.keep, ref)
    np.testing.assert_array_equal(alive[orc.nms(sc.boxes[alive], _scores(len(alive)), S.THRESH, rotated=rotated)], sc.keep)


def test_oracle_iou_on_special_geometry():
    """identical boxes, heading pi, heading pi/2 with swapped dimensions, a contained box, a cross, a shared edge, a corner touch, a
    site at coordinates around 1500: the oracle gives 1, 1, 1, 0.25, 0.2, 0, 0 and 0.4545.  Measured deviation from the closed forms
    on the CPU: 1.4e-8 at the far site (the fp32 rounding of 5 / 11), 3.0e-9 for the cross, 0 for the others -- all below what an fp32
    result near 1 can resolve (half an ulp, 2^-24 = 6.0e-8), so the tolerance is twice that resolution, 1.2e-7."""
    sp = S.special_geometry()
    a = np.array([s[1] for s in sp], np.float32)
    b = np.array([s[2] for s in sp], np.float32)
    want = np.array([s[3] for s in sp])
    got = np.array([orc.boxes_iou_bev(a[k:k + 1], b[k:k + 1])[0, 0] for k in range(len(sp))], np.float64)
    dev = np.abs(got - want)
    print("special geometry: oracle", got, "deviation", dev)
    assert np.all(dev <= 2 * 2.0 ** -24), dev
    assert np.all(got[[1, 2]] == 0.0)                 # a shared edge, a touching corner: exactly nothing
    for na, nb in [(15, 16), (16, 17), (17, 33), (33, 15)]:
        la, lb = S.special_layout(na, nb)
        assert S.tile_edges_nonzero(orc.boxes_iou_bev(la, lb))


@pytest.mark.parametrize("n,rotated", [(200, True), (200, False), (900, True), (900, False)])
def test_oracle_keeps_non_finite_rows_and_they_suppress_nothing(n, rotated):
    """NaN centre, inf length, NaN heading, all-zero box: rotated oracle IoU 0 with everything, themselves included; orc.nms keeps them
    and the fates of all other boxes are those of the scene without them.  The axis-aligned IoU never reads the heading, and its
    fmaxf / fminf drop a NaN operand: a box with a NaN x has the other box's x-interval, IoU 1 with every box on its row of sites, and
    is suppressed by the first of them -- the one fate that differs, and the device chains are held to it (S.nonfinite_keep)."""
    sc = S.nonfinite(n, rotated)
    rows = [p for p in S.NONFINITE_AT if p < n]
    want = S.nonfinite_keep(sc)
    assert not np.all(np.isfinite(sc.boxes[rows[:3]]), axis=1).any() and not sc.boxes[rows[3]].any()
    bb = sc.boxes.copy()
    if not rotated:
        bb[:, 6] = 0
    iou = orc.boxes_iou_bev(bb[rows], bb)
    if rotated:
        assert np.all(iou == 0.0), iou[iou != 0]
    keep = orc.nms(sc.boxes, _scores(n), S.THRESH, rotated=rotated)
    np.testing.assert_array_equal(keep, want)
    if rotated:
        np.testing.assert_array_equal(want, sc.keep)
        assert set(rows) <= set(keep.tolist())
    else:
        assert len(want) == len(sc.keep) - len(rows) // 4
