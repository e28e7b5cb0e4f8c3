"""The three greedy NMS chains -- nms_reduce and topk_chain (csrc/iou3d_nms.hip), step 5 of det_select_nms (csrc/det_post.hip) -- on
scenes whose kept list is known by construction (tests/nms_scenes.py, pinned against a float64 greedy loop and the oracle in
tests/test_nms_scenes_cpu.py): suppressor and victim placed on chosen lanes, words, kept slots and chunk edges, caps inside a word,
words with nothing kept, boxes that were suppressed and must not suppress.  Every IoU of a scene lies at least 0.1 from the threshold,
so the kept lists must be EQUAL: there is no escape clause.  Also the pairwise kernel on special geometry at its tile edges, and
non-finite rows in all three chains against what the oracle does with them."""
import numpy as np
import pytest
import torch

import nms_scenes as S
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROT = [True, False]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scores(n):
    return (n - np.arange(n)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ full chain
def _check_full(boxes, rotated, want):
    from btcdet_amd import iou3d_nms
    keep, cnt = iou3d_nms._nms_sorted(_t(boxes), S.THRESH, rotated)
    got = keep.cpu().numpy()[:cnt]
    assert cnt == len(want), (cnt, len(want), np.setxor1d(got, want)[:20])
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("rotated", ROT)
@pytest.mark.parametrize("n", S.SMALL_N)
def test_full_chain_small_sizes(n, rotated):
    for with_pair in (False, True):
        sc = S.small(n, rotated, with_pair)
        assert len(sc.keep) == n - (1 if with_pair and n >= 2 else 0)
        _check_full(sc.boxes, rotated, sc.keep)


@pytest.mark.parametrize("rotated", ROT)
def test_full_chain_word_edges(rotated):
    sc = S.word_edges(rotated, S.WORD_EDGE_N)
    assert len(sc.keep) == S.WORD_EDGE_N - len(S.WORD_EDGE_PAIRS)
    _check_full(sc.boxes, rotated, sc.keep)


@pytest.mark.parametrize("rotated", ROT)
def test_full_chain_a_suppressed_box_suppresses_nothing(rotated):
    sc = S.triples(rotated)
    kept = set(sc.keep.tolist())
    assert all(a in kept and b not in kept and c in kept for a, b, c in S.TRIPLES)
    _check_full(sc.boxes, rotated, sc.keep)


@pytest.mark.parametrize("rotated", ROT)
def test_full_chain_piles_and_a_word_with_nothing_kept(rotated):
    sc = S.piles(rotated)
    assert not set(range(576, 640)) & set(sc.keep.tolist())
    _check_full(sc.boxes, rotated, sc.keep)


@pytest.mark.parametrize("rotated", ROT)
def test_full_chain_second_trip_of_the_removal_loop(rotated):
    """16 500 boxes are 258 words: from word 0, the 256 threads reach word 257 only on the second trip of `j += 256`"""
    sc = S.long_scene(rotated)
    assert len(sc.keep) == S.LONG_N - len(S.LONG_PAIRS) - len(S.LONG_TRIPLES)
    _check_full(sc.boxes, rotated, sc.keep)


# ----------------------------------------------------------------------------------------------------------------- top-k chain
def _check_topk(scenes, max_keep, rotated):
    from btcdet_amd import iou3d_nms
    boxes = torch.stack([_t(sc.boxes) for sc in scenes])
    keep, cnt = iou3d_nms.nms_topk(boxes, S.THRESH, max_keep, rotated=rotated)
    assert tuple(keep.shape) == (len(scenes), max_keep) and tuple(cnt.shape) == (len(scenes),)
    keep, cnt = keep.cpu().numpy(), cnt.cpu().numpy()
    for s, sc in enumerate(scenes):
        want = sc.keep[:max_keep]
        assert cnt[s] == len(want), (s, cnt[s], len(want), np.setxor1d(keep[s][:cnt[s]], want)[:20])
        np.testing.assert_array_equal(keep[s][:len(want)], want, err_msg="scene %d" % s)
        assert np.all(keep[s][len(want):] == -1), s


@pytest.mark.parametrize("rotated", ROT)
@pytest.mark.parametrize("n", S.CHUNK_N)
def test_topk_chunk_edges(n, rotated):
    """suppressors in kept slots 0, 62 .. 65 of chunk 0, victims at 768, 2303, 2304, 4863, 4864; triples astride the edges"""
    _check_topk([S.chunk_edges(n, 0, rotated), S.chunk_edges(n, 1, rotated)], S.CHUNK_MAX_KEEP, rotated)


@pytest.mark.parametrize("rotated", ROT)
def test_topk_last_kept_slot_across_a_chunk_edge(rotated):
    _check_topk([S.last_slot(v, rotated) for v in (0, 1, 2)], S.LAST_SLOT_MAX_KEEP, rotated)


@pytest.mark.parametrize("rotated", ROT)
@pytest.mark.parametrize("max_keep", S.CAPS)
def test_topk_caps(max_keep, rotated):
    scenes = [S.cap(max_keep, kind, rotated) for kind in S.cap_kinds(max_keep)] + [S.word_edges(rotated, S.CAP_N)]
    _check_topk(scenes, max_keep, rotated)


@pytest.mark.parametrize("rotated", ROT)
def test_topk_4096_slots_fill_over_four_chunks(rotated):
    _check_topk([S.fill4096(0, rotated), S.fill4096(1, rotated)], S.FILL_MAX_KEEP, rotated)


@pytest.mark.parametrize("rotated", ROT)
def test_topk_batch_fills_in_chunk_0_in_chunk_2_and_never(rotated):
    _check_topk([S.three(w, rotated) for w in (1, 2, 0)], S.THREE_MAX_KEEP, rotated)


def test_topk_no_box_and_one_box():
    from btcdet_amd import iou3d_nms
    for max_keep in (1, 64, 100):
        keep, cnt = iou3d_nms.nms_topk(torch.zeros((2, 0, 7), device=DEV), S.THRESH, max_keep)
        assert np.all(keep.cpu().numpy() == -1) and np.all(cnt.cpu().numpy() == 0) and tuple(keep.shape) == (2, max_keep)
        _check_topk([S.small(1, True, True), S.small(1, False, True)], max_keep, True)


# ----------------------------------------------------------------------------------------------------------------- fused chain
def _det_select(cls, boxes, score_thresh, rotated, pre_max, post_max):
    """btc_det_select_nms as post_processing.detect calls it, C = 1, normalized scores -> (keep (B, post_max), num (B,))"""
    from btcdet_amd._lib import check, lib, ptr, stream_ptr, workspace
    L = lib()
    cls, boxes = _t(cls), _t(boxes)
    B, n = int(boxes.shape[0]), int(boxes.shape[1])
    keep = torch.full((B, post_max), -7, dtype=torch.int64, device=DEV)
    num = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    best_class = torch.empty((B, n), dtype=torch.int32, device=DEV)
    ws_bytes = L.btc_det_select_nms_ws_bytes(B, n)
    ws = workspace(ws_bytes, torch.device(DEV))
    check(L.btc_det_select_nms(ptr(cls), ptr(boxes), B, n, 1, 7, 1, float(score_thresh), float(S.THRESH), int(rotated), int(pre_max),
                               int(post_max), ptr(keep), ptr(num), ptr(best_class), ptr(ws), ws_bytes, stream_ptr()), "btc_det_select_nms")
    return keep.cpu().numpy(), num.cpu().numpy()


def _position_scores(m, removed=()):
    sc = (1.0 - np.arange(m) / 2048.0).astype(np.float32)     # distinct, descending with the position, all above 0.5
    sc[list(removed)] = 0.05
    return sc


@pytest.mark.parametrize("rotated", ROT)
@pytest.mark.parametrize("m", S.FUSED_M)
@pytest.mark.parametrize("mode", ["all", "pre_max", "score_thresh", "post_max"])
def test_fused_chain(mode, m, rotated):
    """a batch of two: the scene with its rows in position order, and with its rows permuted (keep holds INPUT indices)"""
    removed = S.FUSED_REMOVED if mode == "score_thresh" else ()
    sc = S.fused(m, rotated, bool(removed))
    pre_max = 700 if mode == "pre_max" else 4096
    post_max = 100 if mode == "post_max" else 1024
    want = sc.keep[sc.keep < pre_max][:post_max]
    assert len(want) == (post_max if mode == "post_max" else len(want)) and len(sc.keep) > 700
    scores = _position_scores(m, removed)
    perm = np.random.default_rng(m).permutation(m)             # input row r holds position perm[r]
    inv = np.argsort(perm)
    cls = np.stack([scores, scores[perm]])[:, :, None]
    boxes = np.stack([sc.boxes, sc.boxes[perm]])
    keep, num = _det_select(cls, boxes, 0.1, rotated, pre_max, post_max)
    for s, w in enumerate([want, inv[want]]):
        assert num[s] == len(w), (s, num[s], len(w))
        np.testing.assert_array_equal(keep[s][:len(w)], w, err_msg="scene %d" % s)
        assert np.all(keep[s][len(w):] == -1), s


# ------------------------------------------------------------------------------------------------------------- pairwise kernel
def test_pairwise_special_geometry_at_tile_edges():
    from btcdet_amd import iou3d_nms
    for na in (15, 16, 17, 33):
        for nb in (15, 16, 17, 33):
            a, b = S.special_layout(na, nb)
            got = iou3d_nms.boxes_iou_bev(_t(a), _t(b)).cpu().numpy()
            assert got.shape == (na, nb) and S.tile_edges_nonzero(got), (na, nb)
            np.testing.assert_allclose(got, orc.boxes_iou_bev(a, b), rtol=1e-4, atol=2e-5, err_msg="%d x %d" % (na, nb))


# ------------------------------------------------------------------------------------------------------------- non-finite rows
@pytest.mark.parametrize("rotated", ROT)
def test_non_finite_rows_in_all_three_chains(rotated):
    """NaN centre, inf length, NaN heading, all-zero box among real candidates: the fates are the oracle's (orc.nms): the rows are kept
    and suppress nothing, their neighbours' fates are unchanged -- but a NaN x in the axis-aligned chain, which fmaxf / fminf drop"""
    for n in (200, 900):
        sc = S.nonfinite(n, rotated)
        want = orc.nms(sc.boxes, _scores(n), S.THRESH, rotated=rotated)
        np.testing.assert_array_equal(want, S.nonfinite_keep(sc))
        _check_full(sc.boxes, rotated, want)
        _check_topk([sc._replace(keep=want), S.word_edges(rotated, 900)] if n == 900 else [sc._replace(keep=want)], 1024, rotated)
        if n == 900:
            _check_topk([S.word_edges(rotated, 900), sc._replace(keep=want)], 64, rotated)
        keep, num = _det_select(_position_scores(n)[None, :, None], sc.boxes[None], 0.1, rotated, 4096, 1024)
        assert num[0] == len(want)
        np.testing.assert_array_equal(keep[0][:len(want)], want)
        assert np.all(keep[0][len(want):] == -1)
