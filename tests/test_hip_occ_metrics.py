"""Occupancy metrics on the GPU (btcdet_amd/occ_metrics.py over csrc/occ_metrics.hip; the occ_metrics switch of btcdet_amd/predictor.py).

Against tests/golden/occ_metrics.npz -- the reference's own Detector3DTemplate.occ_post_processing and eval_utils.get_match_stats -- and, on
seeded cases the golden file does not hold, against the numpy restatement tests/test_occ_metrics_cpu.py pins to that file.  All 16
counters are compared EXACTLY and the float fields bit for bit: every point of those cases lies farther from every face of every valid
box than ten times the reference's own float32 deviation (asserted by the generator and by occ_metrics_ref.seeded_case), except the
on_face case, whose arithmetic is exact.  The masks are handed over as the product hands them over: views into ONE byte arena at offsets
256 + i * vol, which are odd when vol is."""
import numpy as np
import pytest
import torch

import occ_metrics_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
MASKS = ("general_cls_loss_mask", "pos_mask", "neg_mask")


def to_device(bd, prob_offset=0, num_as_tensor=False):
    """numpy batch_dict -> device batch_dict: the three masks as views of one byte arena (offsets 256 + i * vol), the probability
    `prob_offset` floats behind an allocation's start (so that the kernel's head peel runs), pos_all_num a 0-d int32 tensor as OccTargets
    makes it"""
    out = {}
    vol = bd["batch_pred_occ_prob"].size
    arena = torch.full((256 + 3 * vol + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    for k, v in bd.items():
        if k in MASKS:
            view = arena[256 + MASKS.index(k) * vol:256 + (MASKS.index(k) + 1) * vol].view(bd[k].shape)
            view.copy_(torch.from_numpy(np.array(v)))
            out[k] = view
        elif k == "batch_pred_occ_prob":
            buf = torch.full((vol + 8,), float("nan"), dtype=torch.float32, device=DEV)
            out[k] = buf[prob_offset:prob_offset + vol].view(v.shape)
            out[k].copy_(torch.from_numpy(np.array(v)))
        elif k == "pos_all_num":
            out[k] = torch.tensor(v, dtype=torch.int32, device=DEV)
        elif k == "gt_boxes_num" and num_as_tensor:
            out[k] = torch.tensor(v, dtype=torch.int64, device=DEV)
        elif isinstance(v, np.ndarray):
            out[k] = torch.from_numpy(np.array(v)).to(DEV)
        else:
            out[k] = v
    return out


def check_row(got, want, what, boxes=True):
    got = np.asarray(got).tolist()
    print(what, "got", got, "want", np.asarray(want).tolist())
    k = 16 if boxes else 6
    assert got[:k] == np.asarray(want)[:k].tolist(), what


@pytest.fixture(scope="module")
def gold():
    return ref.load_golden()


@pytest.mark.parametrize("name", list(ref.CASES))
def test_against_the_reference_golden_vectors(gold, name):
    from btcdet_amd import occ_metrics as om
    bd = ref.case_inputs(name)
    has = "occ_pnts" in bd
    dbd = to_device(bd)
    before = {k: v.clone() for k, v in dbd.items() if torch.is_tensor(v)}
    row = om.occ_counters(dbd)
    assert row.is_cuda and row.dtype == torch.int64 and row.shape == (16,)
    check_row(row.cpu().numpy(), gold[name + "_counters"], name, boxes=has)
    if not has:       # no points: the boxes still count, nothing is covered
        assert row.cpu().numpy()[6:].tolist() == [sum(bd["gt_boxes_num"])] + [0] * 9
    match, same = om.occ_post_processing(dbd)
    assert same is dbd
    for k, v in zip(("precision", "recall", "f1"), gold[name + "_floats"]):
        assert match[k].dtype == torch.float32 and not match[k].is_cuda and ref.bits(match[k].numpy()) == ref.bits(v), (name, k)
    for k, i in (("total", 0), ("pos_num", 1), ("neg_num", 2), ("pos_all_num", 5)):
        assert match[k].dtype == torch.int64 and int(match[k]) == int(gold[name + "_counters"][i]), (name, k)
    assert ("box_num_sum" in match) == has and ("occ_box_num" in match) == has
    if has:
        assert match["box_num_sum"] == int(gold[name + "_counters"][6]) and match["occ_box_num"] == gold[name + "_counters"][7:].tolist()
    for k, v in before.items():
        assert torch.equal(dbd[k].contiguous().reshape(-1).view(torch.uint8), v.contiguous().reshape(-1).view(torch.uint8)), "input %s was written" % k


# cells: 1, 105, 2 x 105, one workgroup's work -1 / +0 / +1, ~70 001 (several workgroups meet on the atomics); boxes M = 1, 65, 300;
# B = 1, 2, 8; points n = 1, 63, 64, 65 per scene; the probability 1, 2, 3 floats off a 16-byte boundary; points in shuffled scene order
SEEDED = {
    "cell1-m1-n1": dict(seed=101, shape=(1, 1, 1, 1), M=1, num=[1], pts=[1], inside=1.0, prob_offset=1),
    "c105-m65-n63": dict(seed=102, shape=(1, 3, 5, 7), M=65, num=[65], pts=[63], prob_offset=2),
    "c210-b2-m300-n64-65": dict(seed=103, shape=(2, 3, 5, 7), M=300, num=[300, 1], pts=[64, 65], prob_offset=3),
    "c4095-n64": dict(seed=104, shape=(1, 1, 1, ref.BLOCK_CELLS - 1), M=65, num=[64], pts=[64], half=True),
    "c4096-n65": dict(seed=105, shape=(1, 1, 1, ref.BLOCK_CELLS), M=65, num=[65], pts=[65], prob_offset=1, half=True),
    "c4097-n1": dict(seed=106, shape=(1, 1, 1, ref.BLOCK_CELLS + 1), M=1, num=[1], pts=[1], inside=1.0, prob_offset=3, half=True),
    "c70001-b1": dict(seed=107, shape=(1, 1, 1, 70001), M=65, num=[40], pts=[257], prob_offset=2, half=True),
    "b8-m65-shuffled": dict(seed=108, shape=(8, 3, 5, 7), M=65, num=[65, 0, 1, 64, 12, 65, 7, 30], pts=[63, 64, 65, 1, 0, 300, 5, 129], shuffle=True),
    "b8-m300-huge-padding": dict(seed=109, shape=(8, 1, 1, 513), M=300, num=[257, 3, 0, 300, 1, 65, 64, 63], pts=[65, 64, 63, 1, 300, 0, 70, 2],
                                 pad_huge=True),
}


@pytest.mark.parametrize("name", list(SEEDED))
def test_seeded_cases_equal_the_restatement(name):
    from btcdet_amd import occ_metrics as om
    kw = dict(SEEDED[name])
    off, shuffle = kw.pop("prob_offset", 0), kw.pop("shuffle", False)
    bd = ref.seeded_case(**kw)
    if shuffle:       # the order PassOccVox writes is scene by scene; any order is the same computation
        perm = np.random.RandomState(kw["seed"]).permutation(len(bd["occ_pnts"]))
        bd["occ_pnts"], bd["added_occ_b_ind"] = np.ascontiguousarray(bd["occ_pnts"][perm]), bd["added_occ_b_ind"][perm]
    want = ref.counters(bd)
    for as_tensor in (False, True):
        row = om.occ_counters(to_device(bd, prob_offset=off, num_as_tensor=as_tensor))
        check_row(row.cpu().numpy(), want, "%s tensor=%s" % (name, as_tensor))
    assert want[6] == sum(kw["num"]) and (len(kw["num"]) == 1 or want[7] > 0)


def test_out_row_is_overwritten_in_place_and_points_outside_the_batch_take_no_part():
    from btcdet_amd import occ_metrics as om
    bd = dict(ref.case_inputs("c105_b2"))
    want = ref.counters(bd)
    table = torch.full((3, 16), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    # two more points whose scene index is outside 0 .. B-1, inside a box by their coordinates
    inside = bd["gt_boxes"][0, 0, :3]
    bd["occ_pnts"] = np.concatenate([bd["occ_pnts"], np.array([[*inside, 0.99], [*inside, 0.99]], np.float32)])
    bd["added_occ_b_ind"] = np.concatenate([bd["added_occ_b_ind"], np.array([-1, 2], np.int64)])
    row = om.occ_counters(to_device(bd), out=table[1])
    assert row.data_ptr() == table[1].data_ptr()
    t = table.cpu().numpy()
    check_row(t[1], want, "out row")
    assert (t[0] == 0x5A5A5A5A5A5A5A5A).all() and (t[2] == 0x5A5A5A5A5A5A5A5A).all()


def test_occ_counters_reads_nothing_back():
    """occ_counters() and OccEvaluator.add() under torch's sync debug mode "error" raise nothing, with gt_boxes_num as a list and as a
    tensor; an .item() inside that mode does raise on this build (shown first -- otherwise the mode proves nothing and the test skips)"""
    from btcdet_amd import occ_metrics as om
    bd = ref.case_inputs("c105_b2")
    d_list, d_tensor = to_device(bd), to_device(bd, num_as_tensor=True)
    om.occ_counters(d_list)          # (first call: library load, allocator growth)
    ev = om.OccEvaluator(capacity=1)
    probe = torch.ones(4, device=DEV)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.sum().item()
            raised = False
        except RuntimeError:
            raised = True
        if not raised:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag .item() on this build: the mode cannot show the absence of a read-back")
        r1 = om.occ_counters(d_list)
        r2 = om.occ_counters(d_tensor)
        ev.add(d_list)
        ev.add(d_tensor)      # (the table doubles here)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    want = ref.counters(bd)
    for r in (r1, r2, ev.table[0], ev.table[1]):
        check_row(r.cpu().numpy(), want, "under sync debug mode")


def test_evaluator_sums_equal_the_reference_epoch(gold):
    """two add()s then one summary() = the reference's `metric` after two batches; a third add() = after three (bit for bit); the table
    starts at one row here, so it doubles twice"""
    from btcdet_amd import occ_metrics as om
    import test_occ_metrics_cpu as cpu
    ev = om.OccEvaluator(capacity=1)
    batches = [to_device(ref.case_inputs(n)) for n in ref.EPOCH]
    ev.add(batches[0])
    ev.add(batches[1])
    for n in (2, 3):
        assert len(ev) == n
        s = ev.summary()
        fl, ints = cpu.metric_arrays(s["metric"])
        print("after", n, fl.tolist(), ints.tolist())
        assert np.array_equal(ref.bits(fl), ref.bits(gold["epoch%d_floats" % n])) and ints.tolist() == gold["epoch%d_ints" % n].tolist()
        assert len(ev.format()) == 3
        if n == 2:
            ev.add(batches[2])
    assert ev.table.shape[0] == 4
    ev.reset()
    assert len(ev) == 0 and ev.summary()["metric"]["scene_num"] == 0


# ---------------------------------------------------------------------------------------------------------------- BtcPredictor
def test_predictor_with_occ_metrics_on_two_synthetic_batches(monkeypatch, gold):
    """BtcPredictor(model, occ_metrics=True) on the synthetic batches of tests/test_hip_det_post.py: the counters equal the restatement
    applied to the forward's own batch_dict (the real arena-offset masks at the real shape); the default predictor returns what it
    returned and makes no occupancy call.

    For real network outputs no face margin can be asserted: the point-in-box decisions may differ from the float64 restatement only for
    points within the golden file's margin of a face, so occ_box_num has to lie between the restatement with those points excluded and
    with them included.  The cell counters, pos_all_num and box_num_sum stay exact."""
    import det_post_ref
    import test_hip_det_post as tdp
    from btcdet_amd import occ_metrics as om
    from btcdet_amd.predictor import BtcPredictor
    model, batches = tdp._model_and_batches()
    low = tdp.to_cfg(dict(det_post_ref.BASE_CFG, SCORE_THRESH=0.0, NMS_CONFIG=dict(det_post_ref.BASE_CFG["NMS_CONFIG"])))
    margin = max(10.0 * float(gold["deviation"]), 1e-4)
    calls = []
    real = om.occ_counters
    monkeypatch.setattr(om, "occ_counters", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    det = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    recall_keys = {"gt", "roi_0.3", "rcnn_0.3", "roi_0.5", "rcnn_0.5", "roi_0.7", "rcnn_0.7"}
    occ_keys = {"pos_num", "neg_num", "pos_all_num", "total", "precision", "recall", "f1", "box_num_sum", "occ_box_num"}
    try:
        plain, occ = BtcPredictor(model, post_cfg=low), BtcPredictor(model, post_cfg=low, occ_metrics=True)
        assert plain.occ is None and plain.occ_summary() == {} and isinstance(occ.occ, om.OccEvaluator)
        rows = []
        for batch in batches:
            n0 = len(calls)
            want_dicts, want_recall = plain.predict(batch)
            plain(batch)
            assert len(calls) == n0 and set(want_recall) == recall_keys      # the default predictor makes no occupancy call
            got_dicts, got = occ.predict(batch)
            assert len(calls) == n0 + 1 and set(got) == recall_keys | occ_keys
            assert {k: got[k] for k in recall_keys} == want_recall
            for g_, w_ in zip(got_dicts, want_dicts):
                for k in ("pred_boxes", "pred_scores", "pred_labels"):
                    assert torch.equal(g_[k], w_[k]), k
            bd = occ.forward(batch)
            assert bd["general_cls_loss_mask"].dtype == torch.uint8 and "occ_pnts" in bd
            row = real(bd).cpu().numpy()
            assert np.array_equal(row, occ.occ.rows()[-1].numpy()), "predict() recorded another row than the forward's batch_dict gives"
            assert got["occ_box_num"] == row[7:].tolist() and got["box_num_sum"] == int(row[6]) and int(got["total"]) == int(row[0])
            nbd = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in bd.items()
                   if k in MASKS + ("batch_pred_occ_prob", "pos_all_num", "gt_boxes", "gt_boxes_num", "occ_pnts", "added_occ_b_ind", "batch_size")}
            nbd["gt_boxes_num"] = [int(k) for k in np.asarray(nbd["gt_boxes_num"]).reshape(-1)]
            exact, lo, hi = ref.counters(nbd), ref.counters(nbd, slack=-margin), ref.counters(nbd, slack=margin)
            print("cells", nbd["batch_pred_occ_prob"].shape, "points", len(nbd["occ_pnts"]), "boxes", nbd["gt_boxes_num"])
            print("got  ", row.tolist())
            print("exact", exact.tolist(), "lo", lo[7:].tolist(), "hi", hi[7:].tolist())
            assert row[:7].tolist() == exact[:7].tolist()
            assert (lo[7:] <= row[7:]).all() and (row[7:] <= hi[7:]).all()
            assert row[0] > 0 and row[6] > 0
            occ(batch)                       # the resident form adds the batch once more
            assert len(calls) == n0 + 2
            rows += [row, row]
        s = occ.occ_summary()
        assert s["metric"]["scene_num"] == 2 * len(batches)
        want = om.summarize(np.stack(rows))
        assert s["metric"]["total_num_box"] == want["metric"]["total_num_box"] and s["precision"] == want["precision"] and s["f1_factored"] == want["f1_factored"]
    finally:
        torch.use_deterministic_algorithms(det[0], warn_only=det[1])
