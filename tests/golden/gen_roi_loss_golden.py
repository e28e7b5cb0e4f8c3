"""Golden vectors of the ROI head's loss, produced by the reference's OWN RoIHeadTemplate.get_loss (get_box_cls_layer_loss,
get_box_reg_layer_loss with ResidualCoder, WeightedSmoothL1Loss and get_corner_loss_lidar) run here on the CPU through ref_env, over
recorded small inputs (N = B * R <= 64 rois, logits inside +-6).  Per case the inputs, the reference's three terms (class, regression,
corner) and the autograd gradients of its total with respect to rcnn_cls and rcnn_reg are recorded in float32, and the same from float64
inputs.

The reference logs `rcnn_loss_reg` BEFORE it adds the corner term (the repository's torch route logs the sum), so its three terms are
recorded separately: loss = (cls, reg, corner), and the total the gradients belong to is cls + (reg + corner).

The reference's binary_cross_entropy on the CPU refuses a label of -1 ("all elements of target should be between 0 and 1"): the golden
cases therefore carry labels in [0, 1] only, as float32 (CLS_SCORE_TYPE roi_iou).  Ignored labels, int64 labels and the saturation
rules of the class term are checked against the restatement alone (tests/roi_loss_ref.py).  The reference computes the corner term
only when there is a foreground roi; with none it records 0, which is what a masked sum gives.  It clamps the caller's gt_of_rois dims
in place (encode_torch on a view): every run below gets clones.  It casts the labels and the rotation matrix of
rotate_points_along_z with `.float()` whatever the input type, which binary_cross_entropy and matmul refuse beside a double operand:
for the float64 run alone `Tensor.float()` leaves a DOUBLE tensor as it is (masks and integers convert as always), nothing else is
touched.

Every case keeps the margins of roi_loss_ref.assert_margins (ties of a corner's two distances, trig arguments, logits).

    python tests/golden/gen_roi_loss_golden.py   ->  tests/golden/roi_loss.npz"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_env  # noqa: E402
import oracle_spconv  # noqa: E402

ref_env.install(oracle_spconv)
import torch  # noqa: E402

import roi_loss_ref as rl  # noqa: E402
from btcdet.models.roi_heads.roi_head_template import RoIHeadTemplate  # noqa: E402

F = np.float32

# name, scenes, rois per scene, the roi_loss_ref value kind its inputs are built from, corner term
CASES = [
    dict(name="b2_mixed", B=2, R=16, kind="random", corner=True),
    dict(name="b1_no_fg", B=1, R=24, kind="no_fg", corner=True),
    dict(name="b3_all_fg", B=3, R=8, kind="all_fg", corner=True),
    dict(name="b2_twin", B=2, R=32, kind="twin_nearer", corner=True),
    dict(name="b2_no_corner", B=2, R=16, kind="random", corner=False),
    dict(name="b2_tiny_dims", B=2, R=24, kind="tiny_dims", corner=True),
    dict(name="b1_nan_target", B=1, R=32, kind="nan_target", corner=True),
    dict(name="b2_dist_one", B=2, R=12, kind="dist_one", corner=True),
]


def ref_head(corner):
    cfg = ref_env.load_ref_cfg().MODEL.ROI_HEAD
    cfg.LOSS_CONFIG.CORNER_LOSS_REGULARIZATION = bool(corner)
    cfg.LOSS_CONFIG.LOSS_WEIGHTS.update(rl.W_DEFAULT)
    assert cfg.LOSS_CONFIG.CLS_LOSS == "BinaryCrossEntropy" and cfg.LOSS_CONFIG.REG_LOSS == "smooth-l1"
    head = RoIHeadTemplate(num_class=1, model_cfg=cfg)
    head.build_losses(cfg.LOSS_CONFIG)
    return head


def ref_loss(head, d, B, dtype):
    """the reference's get_loss and the autograd gradients of its total -> (loss (3) = cls, reg, corner; d_cls (N,); d_reg (N, 7))"""
    N = d["mask"].size
    R = N // B
    t = lambda a, *shape: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).view(*shape).clone()
    cls, reg = t(d["cls"], N, 1).requires_grad_(True), t(d["reg"], N, 7).requires_grad_(True)
    head.forward_ret_dict = dict(rois=t(d["rois"], B, R, 7), gt_of_rois=t(d["gt"], B, R, 8), gt_of_rois_src=t(d["src"], B, R, 8),
                                 reg_valid_mask=torch.from_numpy(d["mask"].copy()).view(B, R), rcnn_cls_labels=t(d["labels"], B, R), rcnn_cls=cls, rcnn_reg=reg)
    to_float = torch.Tensor.float
    if dtype is torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self if self.dtype == torch.float64 else to_float(self, *a, **k)
    try:
        loss, tb = head.get_loss()
    finally:
        torch.Tensor.float = to_float
    loss.backward()
    out = np.array([tb["rcnn_loss_cls"], tb["rcnn_loss_reg"], tb.get("rcnn_loss_corner", 0.0)], np.float64)
    assert abs(float(loss.detach()) - out.sum()) <= 1e-5 * max(abs(float(loss.detach())), 1.0)
    return out, cls.grad.numpy().reshape(N), reg.grad.numpy().reshape(N, 7)


if __name__ == "__main__":
    gold, index = {}, []
    for c in CASES:
        name, B, R = c["name"], c["B"], c["R"]
        d = rl.make_case(dict(N=B * R, kind=c["kind"], labels="roi_iou", corner=c["corner"], gold=name), poison=False)
        d["cls"] = np.clip(d["cls"], -6, 6)
        d["B"] = B
        m = rl.assert_margins(d)
        assert B * R <= 64 and d["labels"].dtype == F and d["labels"].min() >= 0 and d["labels"].max() <= 1
        head = ref_head(c["corner"])
        for key, shape in (("cls", (B * R,)), ("reg", (B * R, 7)), ("rois", (B, R, 7)), ("gt", (B, R, 8)), ("src", (B, R, 8)), ("labels", (B, R))):
            gold[name + "/" + key] = d[key].reshape(shape)
        gold[name + "/mask"] = d["mask"].reshape(B, R).astype(np.int8)
        before = {k: d[k].copy() for k in ("cls", "reg", "rois", "gt", "src", "labels")}
        o32, c32, r32 = ref_loss(head, d, B, torch.float32)
        o64, c64, r64 = ref_loss(head, d, B, torch.float64)
        assert all(np.array_equal(before[k], d[k], equal_nan=True) for k in before), "the reference wrote the recorded inputs"
        assert np.isfinite(o32).all() and np.isfinite(o64).all() and r64.dtype == np.float64, name
        gold[name + "/loss32"], gold[name + "/d_cls32"], gold[name + "/d_reg32"] = o32.astype(F), c32, r32
        gold[name + "/loss64"], gold[name + "/d_cls64"], gold[name + "/d_reg64"] = o64, c64, r64
        # the restatement against the reference's float64 record, here where both run
        Rs = rl.restate(d, own=True)
        worst = 0.0
        for got, ref in ((Rs["out"][:3], o64), (Rs["d_cls"], c64), (Rs["d_reg"], r64)):
            err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
            assert np.isfinite(ref).all() and np.isfinite(got).all(), name
            worst = max(worst, float(np.where(ref == 0, np.where(got == 0, 0.0, np.inf), err).max()))
        assert worst < 1e-12, (name, worst)
        print("%-16s B %d R %2d corner %-5s foreground %2d  tie margin %.3g  |m - 1| %.3g  restatement vs f64 record %.1e  loss %s" %
              (name, B, R, c["corner"], int((d["mask"] > 0).sum()), m["tie"], m["one"], worst, np.round(o32, 5)))
        index.append(dict(name=name, B=B, R=R, corner=c["corner"], kind=c["kind"]))
    gold["cases"] = np.array(json.dumps(index))
    path = os.path.join(HERE, "roi_loss.npz")
    np.savez_compressed(path, **gold)
    print("wrote roi_loss.npz %.0f KB" % (os.path.getsize(path) / 1024))
