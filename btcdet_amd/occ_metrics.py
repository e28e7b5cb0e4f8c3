"""Occupancy metrics of the eval forward: the reference's ``Detector3DTemplate.occ_post_processing`` (detector3d_template.py:479-546)
and the epoch side of it, ``eval_utils.get_match_stats`` (eval_utils.py:23-39) with the three log lines of eval_utils.py:156-163.

The reference reduces the occupancy grid five times, then walks the scenes in Python -- a 4x4 ``torch.inverse``, an ``(N, M, 3)`` einsum --
and, for each of nine thresholds and every scene, runs a ``nonzero``, a gather, a ``max`` and one ``.item()``.  Here a batch is ONE call of
libbtcdet_hip.so, ``btc_occ_metrics`` (csrc/occ_metrics.hip: a memset and two launches), which leaves a row of 16 exact int64 counters on
the device:

    [total, pos_num, neg_num, pos_predict, pos_correct, pos_all_num, box_num_sum, occ_box_num[0..8]]

``occ_counters`` reads nothing back.  ``occ_post_processing`` gives the reference's ``match_dicts`` with ONE copy to the host; its float
fields are formed on the host from the counters with the reference's own float32 operations, so they carry the reference's bits.
``OccEvaluator`` keeps one row per batch in a device table and reads it once, in ``summary()``.  There is no fallback: a missing kernel
is an error."""
import torch

from ._lib import check, lib, ptr, stream_ptr, workspace

N_COUNTERS = 16
TOTAL, POS_NUM, NEG_NUM, POS_PREDICT, POS_CORRECT, POS_ALL_NUM, BOX_NUM_SUM, OCC_BOX_NUM = 0, 1, 2, 3, 4, 5, 6, 7
THRESHOLDS = tuple(range(1, 10))          # i: probability >= float32(i * 0.1)


def _bytes(t):
    """a 0 / 1 mask as contiguous bytes, without a copy where it already is one (bool and int8 share uint8's memory)"""
    if t.dtype in (torch.bool, torch.int8):
        t = t.view(torch.uint8)
    elif t.dtype != torch.uint8:
        t = (t != 0).view(torch.uint8)
    return t if t.is_contiguous() else t.contiguous()


def _int32_on(v, dev):
    """counts (a list, an int or a tensor) -> int32 [n] on the device; a host value goes up through pinned memory without blocking"""
    if torch.is_tensor(v) and v.is_cuda:
        return v.detach().reshape(-1).to(torch.int32).contiguous()
    if not torch.is_tensor(v):
        v = torch.tensor([int(x) for x in v] if hasattr(v, "__len__") else [int(v)])
    return v.detach().reshape(-1).to(torch.int32).pin_memory().to(dev, non_blocking=True)


@torch.no_grad()
def occ_counters(batch_dict, out=None):
    """-> the int64 [16] row of this batch on the device (`out` when given: a contiguous int64 [16] view, fully overwritten); nothing is
    read back.  Without `occ_pnts` in the batch the box counters are computed from no points (box_num_sum still counts the boxes when
    gt_boxes / gt_boxes_num are there)."""
    prob = batch_dict["batch_pred_occ_prob"].detach()
    dev = prob.device
    if prob.dtype != torch.float32 or not prob.is_contiguous():
        prob = prob.float().contiguous()
    cls, pos, neg = (_bytes(batch_dict[k]) for k in ("general_cls_loss_mask", "pos_mask", "neg_mask"))
    n_cells = prob.numel()
    assert cls.numel() == n_cells and pos.numel() == n_cells and neg.numel() == n_cells, "the masks and batch_pred_occ_prob differ in size"
    pos_all = _int32_on(batch_dict["pos_all_num"], dev)
    pnts = b_ind = gt = gtn = None
    B = M = stride = n_pts = 0
    if batch_dict.get("gt_boxes", None) is not None and batch_dict.get("gt_boxes_num", None) is not None:
        gt = batch_dict["gt_boxes"].detach()
        if gt.dtype != torch.float32 or not gt.is_contiguous():
            gt = gt.float().contiguous()
        B, M, stride = int(gt.shape[0]), int(gt.shape[1]), int(gt.shape[2])
        gtn = _int32_on(batch_dict["gt_boxes_num"], dev)
        assert gtn.numel() == B, "gt_boxes_num has %d entries for %d scenes" % (gtn.numel(), B)
    if "occ_pnts" in batch_dict:
        assert gt is not None, "occ_pnts without gt_boxes / gt_boxes_num"
        pnts = batch_dict["occ_pnts"].detach()
        if pnts.dtype != torch.float32 or not pnts.is_contiguous():
            pnts = pnts.float().contiguous()
        assert pnts.dim() == 2 and pnts.shape[1] == 4, "occ_pnts is (n, 4): x y z probability"
        b_ind = batch_dict["added_occ_b_ind"].detach().reshape(-1)
        if b_ind.dtype != torch.int64 or not b_ind.is_contiguous():
            b_ind = b_ind.to(torch.int64).contiguous()
        n_pts = int(pnts.shape[0])
        assert b_ind.numel() == n_pts
    if out is None:
        out = torch.empty((N_COUNTERS,), dtype=torch.int64, device=dev)
    assert out.dtype == torch.int64 and out.numel() == N_COUNTERS and out.is_contiguous() and out.device == dev
    L = lib()
    ws_bytes = L.btc_occ_metrics_ws_bytes(B, M)
    ws = workspace(ws_bytes, dev)
    check(L.btc_occ_metrics(ptr(prob), ptr(cls), ptr(pos), ptr(neg), n_cells, ptr(pos_all), ptr(pnts) if n_pts else None,
                            ptr(b_ind) if n_pts else None, n_pts, ptr(gt) if B * M else None, ptr(gtn), B, M, stride, ptr(out), ptr(ws), ws_bytes,
                            stream_ptr()), "btc_occ_metrics")
    return out


def match_dicts_from(row, with_boxes=True):
    """one row of 16 host counters (int64 tensor / array / list) -> the reference's match_dicts: CPU tensors of the reference's types, the
    float fields by the reference's float32 arithmetic (call_precision_recall_f1: int64 -> float32, clamp(min=1.0), divide; the 1e-8 clamp
    of F1); `box_num_sum` an int and `occ_box_num` a list of nine ints, absent without `with_boxes`"""
    c = torch.as_tensor(row, dtype=torch.int64).reshape(-1)
    assert c.numel() == N_COUNTERS
    pos_num, pos_predict, pos_correct = c[POS_NUM].clone(), c[POS_PREDICT].clone(), c[POS_CORRECT].clone()
    precision = pos_correct / torch.clamp(pos_predict, min=1.0)
    recall = pos_correct / torch.clamp(pos_num, min=1.0)
    f1 = 2 * precision * recall / torch.clamp(precision + recall, min=1e-8)
    d = {"pos_num": pos_num, "neg_num": c[NEG_NUM].clone(), "pos_all_num": c[POS_ALL_NUM].clone(), "total": c[TOTAL].clone(),
         "precision": precision, "recall": recall, "f1": f1}
    if with_boxes:
        d["box_num_sum"] = int(c[BOX_NUM_SUM])
        d["occ_box_num"] = [int(v) for v in c[OCC_BOX_NUM:OCC_BOX_NUM + 9]]
    return d


@torch.no_grad()
def occ_post_processing(batch_dict):
    """-> (match_dicts, batch_dict) as the reference's occ_post_processing, from occ_counters() with ONE copy to the host"""
    row = occ_counters(batch_dict).cpu()                                                  # the read-back
    return match_dicts_from(row, with_boxes="occ_pnts" in batch_dict), batch_dict


def _new_metric():
    m = {"scene_num": 0, "scene_total_factor": 0, "precision": 0, "recall": 0, "f1": 0, "precision_factored": 0, "recall_factored": 0,
         "f1_factored": 0, "total_num_box": 0, "total_pos_all_portion": 0}
    for i in THRESHOLDS:
        m["total_occ_num_box_%.1f" % (i * 0.1)] = 0
    return m


def accumulate(metric, ret):
    """one batch's match_dicts into the epoch's `metric`, in the reference's order of operations (get_match_stats): torch CPU scalars, so
    the sums carry the reference's bits.  A batch without the box keys adds no boxes."""
    factor = ret["total"] / 1000.0
    metric["scene_total_factor"] += factor
    metric["scene_num"] += 1
    for k in ("precision", "recall", "f1"):
        metric[k] += ret[k]
    for k in ("precision", "recall", "f1"):
        metric[k + "_factored"] += ret[k] * factor
    metric["total_pos_all_portion"] += ret["pos_num"] / max(1.0, ret["pos_all_num"])
    if "box_num_sum" in ret:
        metric["total_num_box"] += ret["box_num_sum"]
        for i in THRESHOLDS:
            metric["total_occ_num_box_%.1f" % (i * 0.1)] += ret["occ_box_num"][i - 1]
    return metric


RATIOS = ("precision", "recall", "f1", "precision_factored", "recall_factored", "f1_factored")


def summarize(rows, with_boxes=None):
    """host rows [n][16] in batch order -> {"metric": the reference's `metric` entries (its sums, torch CPU scalars and ints), and the
    ratios of its three log lines as floats: precision .. f1_factored, occ_thresh_0.1 .. occ_thresh_0.9, total_pos_all_portion}"""
    metric = _new_metric()
    rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1, N_COUNTERS)
    for k in range(rows.shape[0]):
        accumulate(metric, match_dicts_from(rows[k], with_boxes=True if with_boxes is None else bool(with_boxes[k])))
    out = {"metric": metric}
    if metric["scene_num"] == 0:
        return out
    for k in RATIOS:
        out[k] = float(metric[k] / metric["scene_total_factor" if k.endswith("_factored") else "scene_num"])
    for i in THRESHOLDS:
        key = "%.1f" % (i * 0.1)
        out["occ_thresh_" + key] = metric["total_occ_num_box_" + key] / metric["total_num_box"] if metric["total_num_box"] else float("nan")
    out["total_pos_all_portion"] = float(metric["total_pos_all_portion"] / metric["scene_num"])
    return out


def format_summary(s):
    """the three lines the reference logs at the end of an epoch, as it words them"""
    if not s["metric"]["scene_num"]:
        return []
    return [" ".join(["precision: %.3f, recall: %.3f," % (s["precision"], s["recall"]),
                      "f1: %.3f, precision_factored: %.3f" % (s["f1"], s["precision_factored"]),
                      "recall_factored: %.3f, f1_factored: %.3f" % (s["recall_factored"], s["f1_factored"])]),
            " ".join(["occ thresh %.1f: %.3f,  " % (i * 0.1, s["occ_thresh_%.1f" % (i * 0.1)]) for i in THRESHOLDS]),
            " total_pos_all_portion %.3f" % s["total_pos_all_portion"]]


class OccEvaluator(object):
    """The epoch side: add(batch_dict) writes the batch's 16 counters into a device table that grows by doubling (no read-back);
    summary() reads the table once and replays the reference's accumulation in batch order."""

    def __init__(self, capacity=64):
        self._cap0 = max(int(capacity), 1)
        self.reset()

    def reset(self):
        self.table = None
        self.n = 0
        self._boxes = []          # per batch: whether it carried occ_pnts (host knowledge, no read-back)

    def _row(self, dev):
        if self.table is None:
            self.table = torch.empty((self._cap0, N_COUNTERS), dtype=torch.int64, device=dev)
        elif self.n == self.table.shape[0]:
            grown = torch.empty((2 * self.n, N_COUNTERS), dtype=torch.int64, device=dev)
            grown[:self.n].copy_(self.table)
            self.table = grown
        return self.table[self.n]

    def add(self, batch_dict):
        """-> this batch's row (a view of the table, resident)"""
        row = occ_counters(batch_dict, out=self._row(batch_dict["batch_pred_occ_prob"].device))
        self._boxes.append("occ_pnts" in batch_dict)
        self.n += 1
        return row

    def __len__(self):
        return self.n

    def rows(self):
        """the table's filled part on the host: the one read-back"""
        if self.n == 0:
            return torch.zeros((0, N_COUNTERS), dtype=torch.int64)
        return self.table[:self.n].cpu()

    def summary(self):
        return summarize(self.rows(), self._boxes)

    def format(self):
        return format_summary(self.summary())
