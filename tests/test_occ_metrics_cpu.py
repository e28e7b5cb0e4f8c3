"""Occupancy metrics, the parts that need no GPU: the numpy restatement (tests/occ_metrics_ref.py) equals the reference's own results
(tests/golden/occ_metrics.npz) on every golden case -- integers exactly, float fields bit for bit --, and the host side of
btcdet_amd/occ_metrics.py (the float formation and the epoch replay), fed the golden counters, gives the reference's match_dicts and
`metric` bit for bit."""
import numpy as np
import pytest
import torch

import occ_metrics_ref as ref

FLOAT_KEYS = ["scene_total_factor", "precision", "recall", "f1", "precision_factored", "recall_factored", "f1_factored", "total_pos_all_portion"]


@pytest.fixture(scope="module")
def gold():
    return ref.load_golden()


def metric_arrays(metric):
    ints = [metric["scene_num"], metric["total_num_box"]] + [metric["total_occ_num_box_%.1f" % (i * 0.1)] for i in range(1, 10)]
    return np.array([float(metric[k]) for k in FLOAT_KEYS], np.float32), np.array([int(v) for v in ints], np.int64)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_restatement_equals_the_reference(gold, name):
    bd = ref.case_inputs(name)
    c = ref.counters(bd)
    k = 16 if "occ_pnts" in bd else 6          # without occupancy points the reference hands out no box counts
    assert c.dtype == np.int64 and c[:k].tolist() == gold[name + "_counters"][:k].tolist(), (name, c.tolist(), gold[name + "_counters"].tolist())
    assert np.array_equal(ref.bits(ref.floats(c)), ref.bits(gold[name + "_floats"])), name
    assert bool(gold[name + "_has_boxes"]) == ("occ_pnts" in bd)


def test_golden_file_holds_the_margin_it_was_generated_under(gold):
    dev = float(gold["deviation"])
    assert 0.0 < dev and max(10.0 * dev, 1e-4) < ref.SAMPLE_MARGIN
    for name in ref.CASES:
        bd = ref.case_inputs(name)
        if name in ref.MARGIN_EXEMPT or "occ_pnts" not in bd:
            continue
        for b in range(bd["batch_size"]):
            p = bd["occ_pnts"][bd["added_occ_b_ind"] == b]
            d = ref.face_distance(p, bd["gt_boxes"][b, :bd["gt_boxes_num"][b]])
            assert len(d) == 0 or d.min() > max(10.0 * dev, 1e-4), (name, b)


def test_thresholds_are_the_float32_values_torch_compares_with():
    """float32(0.7) and float32(0.9) lie BELOW the doubles 7 * 0.1 and 9 * 0.1; torch compares a float32 tensor with the scalar in float32"""
    for i in range(1, 10):
        t = torch.tensor([ref.THRESH32[i - 1]], dtype=torch.float32)
        assert bool((t >= i * 0.1).all()), i
        assert not bool((torch.tensor([ref.below(ref.THRESH32[i - 1])]) >= i * 0.1).any()), i
    assert float(ref.THRESH32[6]) < 7 * 0.1 and float(ref.THRESH32[8]) < 9 * 0.1


@pytest.mark.parametrize("name", list(ref.CASES))
def test_host_float_formation_equals_the_reference(gold, name):
    from btcdet_amd import occ_metrics as om
    has = bool(gold[name + "_has_boxes"])
    d = om.match_dicts_from(gold[name + "_counters"], with_boxes=has)
    for k, v in zip(("precision", "recall", "f1"), gold[name + "_floats"]):
        assert d[k].dtype == torch.float32 and d[k].dim() == 0 and not d[k].is_cuda
        assert ref.bits(d[k].numpy()) == ref.bits(v), (name, k, float(d[k]), float(v))
    c = gold[name + "_counters"]
    for k, i in (("total", 0), ("pos_num", 1), ("neg_num", 2), ("pos_all_num", 5)):
        assert d[k].dtype == torch.int64 and d[k].dim() == 0 and int(d[k]) == int(c[i])
    assert ("box_num_sum" in d) == has and ("occ_box_num" in d) == has
    if has:
        assert isinstance(d["box_num_sum"], int) and d["box_num_sum"] == int(c[6])
        assert d["occ_box_num"] == [int(v) for v in c[7:]] and all(isinstance(v, int) for v in d["occ_box_num"])


def test_epoch_replay_equals_the_reference(gold):
    from btcdet_amd import occ_metrics as om
    rows = np.stack([gold[name + "_counters"] for name in ref.EPOCH])
    for n in (2, 3):
        s = om.summarize(rows[:n])
        fl, ints = metric_arrays(s["metric"])
        assert np.array_equal(ref.bits(fl), ref.bits(gold["epoch%d_floats" % n])), (n, fl.tolist(), gold["epoch%d_floats" % n].tolist())
        assert ints.tolist() == gold["epoch%d_ints" % n].tolist()
        m = s["metric"]
        for k in FLOAT_KEYS:
            assert torch.is_tensor(m[k]) and m[k].dtype == torch.float32
        # the ratios of the three log lines
        assert s["precision"] == float(m["precision"] / m["scene_num"]) and s["f1_factored"] == float(m["f1_factored"] / m["scene_total_factor"])
        assert s["total_pos_all_portion"] == float(m["total_pos_all_portion"] / m["scene_num"])
        for i in range(1, 10):
            assert s["occ_thresh_%.1f" % (i * 0.1)] == m["total_occ_num_box_%.1f" % (i * 0.1)] / m["total_num_box"]
        lines = om.format_summary(s)
        assert len(lines) == 3
        assert lines[0] == "precision: %.3f, recall: %.3f, f1: %.3f, precision_factored: %.3f recall_factored: %.3f, f1_factored: %.3f" % tuple(
            s[k] for k in om.RATIOS)
        assert lines[1].startswith("occ thresh 0.1: %.3f,   occ thresh 0.2: " % s["occ_thresh_0.1"]) and lines[1].count("occ thresh") == 9
        assert lines[2] == " total_pos_all_portion %.3f" % s["total_pos_all_portion"]


def test_empty_evaluator_and_growth_bookkeeping():
    from btcdet_amd import occ_metrics as om
    ev = om.OccEvaluator()
    assert len(ev) == 0 and ev.summary()["metric"]["scene_num"] == 0 and ev.format() == []
    s = om.summarize(np.zeros((0, 16), np.int64))
    assert set(s) == {"metric"}
    # a batch without occupancy points adds no boxes (the reference's match_dicts has no box keys then)
    row = np.arange(1, 17, dtype=np.int64)
    assert om.summarize(row, with_boxes=[False])["metric"]["total_num_box"] == 0
    assert om.summarize(row, with_boxes=[True])["metric"]["total_num_box"] == 7


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """negative sizes, missing required pointers and a short workspace are BTC_EINVAL with a message; the (never dereferenced) pointers
    are not device memory"""
    from btcdet_amd import _lib
    L = _lib.lib()
    p = 0x1000
    need = L.btc_occ_metrics_ws_bytes(2, 5)
    assert need >= 512 + 2 * 5 * 4 and L.btc_occ_metrics_ws_bytes(0, 0) == 512 and L.btc_occ_metrics_ws_bytes(-1, 7) == 512

    def call(prob=p, cls=p, pos=p, neg=p, n_cells=10, pos_all=p, pnts=p, bind=p, n_pts=3, gt=p, gtn=p, B=2, M=5, stride=8, out=p, ws=p, ws_bytes=need):
        return L.btc_occ_metrics(prob, cls, pos, neg, n_cells, pos_all, pnts, bind, n_pts, gt, gtn, B, M, stride, out, ws, ws_bytes, None)

    for kw in (dict(n_cells=-1), dict(n_pts=-1), dict(B=-1), dict(M=-1), dict(prob=None), dict(cls=None), dict(pos=None), dict(neg=None),
               dict(pos_all=None), dict(pnts=None), dict(bind=None), dict(gt=None), dict(gtn=None), dict(stride=6), dict(out=None), dict(ws=None),
               dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(prob=p + 2), dict(pnts=p + 4)):
        assert call(**kw) == -1, kw
        assert L.btc_last_error().startswith(b"btc_occ_metrics"), kw
