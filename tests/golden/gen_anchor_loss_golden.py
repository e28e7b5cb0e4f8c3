"""Golden vectors of the anchor head's loss, produced by the reference's OWN AnchorHeadTemplate.get_loss (get_cls_layer_loss,
get_box_reg_layer_loss with the loss modules of utils/loss_utils.py) run here on the CPU through ref_env, over recorded small inputs on
the two heads of anchor_loss_ref.GOLD_MAPS.  Per case the inputs, the four loss values (cls, loc, dir, total) and the autograd gradients
of the total with respect to the three prediction tensors are recorded in float32, and the same from float64 inputs.

The reference's functions accept double inputs, with one reservation: they form the anchor weights 1 / n_b in FLOAT32 whatever the input
type.  The float64 record is therefore float64-accurate only where 1 / n_b is a float32 number, and the cases that carry one keep every
scene's positive count a power of two (asserted below); `three_odd_counts` has counts 5 and 11 and is recorded in float32 only.
Logits stay inside +-6, so that the reference's 1 - sigmoid(x) keeps twelve digits in float64.

Direction inputs keep a margin of 1e-4 around an integer bin quotient (anchor_loss_ref.margins_dir, asserted), except the one anchor of
`car_on_clamp` that is MEANT to sit just below a whole turn, where the float32 quotient reaches `bins` and the clamp brings it back.
Nothing the labels exclude holds NaN here: the reference multiplies those entries by a zero weight.  The NaN regression targets sit in
columns 0..5: a NaN HEADING target makes the reference's own loss NaN (its prediction side sin(p) cos(t) is NaN too), so there is
nothing to record for it; the header's rule (the column contributes 0) is checked against the restatement alone.

    python tests/golden/gen_anchor_loss_golden.py   ->  tests/golden/anchor_loss.npz"""
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

import anchor_loss_ref as al  # noqa: E402
from btcdet.models.dense_heads.anchor_head_template import AnchorHeadTemplate  # noqa: E402

F = np.float32

# name, map, per scene (positives, ignored: "some" / "all" / "none"), direction classifier, options
CASES = [
    dict(name="car_dir_b1", map="car", scenes=[(8, "some")], dir=True),
    dict(name="car_dir_b3_mixed", map="car", scenes=[(16, "some"), (0, "some"), (1, "none")], dir=True),        # the clamp max(n, 1); one positive
    dict(name="car_nodir_b2_ignored", map="car", scenes=[(4, "some"), (0, "all")], dir=False),                  # a scene of ignored anchors only
    dict(name="three_dir_b3_nan", map="three", scenes=[(32, "some"), (4, "none"), (2, "some")], dir=True, nan=(2, 5)),
    dict(name="three_nodir_b1_nan", map="three", scenes=[(16, "some")], dir=False, nan=(0, 5, 3)),
    dict(name="car_on_clamp", map="car", scenes=[(2, "some"), (8, "none")], dir=True, clamp=True),
    dict(name="three_odd_counts", map="three", scenes=[(5, "some"), (11, "some")], dir=True, f64=False),
]


def ref_head(map_name, with_dir):
    m = al.GOLD_MAPS[map_name]
    cfg = ref_env.EasyDict(json.loads(json.dumps(al.gold_cfg(map_name, with_dir))))
    head = AnchorHeadTemplate(cfg, num_class=len(m["class_names"]), class_names=m["class_names"], grid_size=np.array(m["grid_size"]),
                              point_cloud_range=np.array(m["point_cloud_range"], F), predict_boxes_when_training=False)
    head.num_anchors_per_location = sum(head.num_anchors_per_location)          # as AnchorHeadSingle.__init__ does
    return head


def ref_loss(head, d, dtype):
    """the reference's get_loss and the autograd gradients of its total -> (loss (4), d_cls, d_box, d_dir or None)"""
    B, A = d["labels"].shape
    per = head.num_anchors_per_location
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    cls = t(d["cls"]).view(B, A // per, -1).requires_grad_(True)
    box = t(d["box"]).view(B, A // per, -1).requires_grad_(True)
    f = dict(cls_preds=cls, box_preds=box, box_cls_labels=torch.from_numpy(d["labels"].copy()), box_reg_targets=t(d["tgt"]))
    if d["dir"] is not None:
        f["dir_cls_preds"] = t(d["dir"]).view(B, A // per, -1).requires_grad_(True)
    head.forward_ret_dict = f
    loss, tb = head.get_loss()
    loss.backward()
    out = np.array([tb["rpn_loss_cls"], tb["rpn_loss_loc"], tb.get("rpn_loss_dir", 0.0), tb["rpn_loss"]], np.float64)
    nd = lambda x, w: x.grad.numpy().reshape(B, A, w)
    return out, nd(cls, d["cls"].shape[2]), nd(box, 7), (nd(f["dir_cls_preds"], d["dir"].shape[2]) if d["dir"] is not None else None)


def build(c, anchors):
    rng = np.random.default_rng(al._seed("gold", c["name"]))
    B, A = len(c["scenes"]), anchors.shape[0]
    C = len(al.GOLD_MAPS[c["map"]]["class_names"])
    labels = np.zeros((B, A), np.int32)
    for b, (npos, ign) in enumerate(c["scenes"]):
        order = rng.permutation(A)
        labels[b, order[:npos]] = rng.integers(1, 4, npos)                      # class ids 1..3 on either head
        rest = order[npos:]
        if ign == "all":
            labels[b, rest] = -1
        elif ign == "some":
            labels[b, rest[:len(rest) // 10]] = -1
    cls = np.clip(rng.standard_normal((B, A, C)) * 2, -6, 6).astype(F)
    box = (rng.standard_normal((B, A, 7)) * 0.4).astype(F)
    tgt = (box + rng.standard_normal((B, A, 7)) * 0.15).astype(F)
    tgt[..., 6] = rng.uniform(-np.pi, np.pi, (B, A)).astype(F)
    box[..., 6] = (tgt[..., 6] + rng.standard_normal((B, A)) * 0.2).astype(F)
    dirs = rng.standard_normal((B, A, 2)).astype(F) if c["dir"] else None
    d = dict(cls=cls, box=box, dir=dirs, labels=labels, tgt=tgt, anchors=anchors, w=dict(al.W_DEFAULT), dir_offset=al.DIR_OFFSET)
    al.clear_dir_margins(d)
    on_clamp = None
    if c.get("clamp"):
        b, a = 0, int(np.flatnonzero(labels[0] > 0)[0])
        t6 = F(al.DIR_OFFSET) - anchors[a, 6]
        for _ in range(4):
            t6 = np.nextafter(t6, F(-4))
        tgt[b, a, 6] = t6                                                        # rot - dir_offset a few 1e-7 below 0: lp rounds to 2 pi
        on_clamp = np.zeros((B, A), bool)
        on_clamp[b, a] = True
    if c.get("nan"):
        b = 0
        rows = np.flatnonzero(labels[b] > 0)[:len(c["nan"])]
        for a, k in zip(rows, c["nan"]):
            tgt[b, a, k] = np.nan
    al.margins_dir(d, on_clamp=on_clamp)
    return d, on_clamp


if __name__ == "__main__":
    gold, index = {}, []
    for c in CASES:
        name, with_f64 = c["name"], c.get("f64", True)
        head = ref_head(c["map"], c["dir"])
        anchors = torch.cat(head.anchors, dim=-3).view(-1, 7).numpy().astype(F)
        d, on_clamp = build(c, anchors)
        counts = (d["labels"] > 0).sum(1)
        assert [int(n) for n in counts] == [s[0] for s in c["scenes"]]
        if with_f64:
            assert all(n == 0 or (n & (n - 1)) == 0 for n in counts), "a float64 record needs power-of-two positive counts"
        assert anchors.shape[0] <= 1530
        for key in ("cls", "box", "tgt", "anchors", "labels"):
            gold[name + "/" + key] = d[key].astype(np.int8) if key == "labels" else d[key]
        if c["dir"]:
            gold[name + "/dir"] = d["dir"]
        o32, c32, b32, d32 = ref_loss(head, d, torch.float32)
        assert np.isfinite(o32).all(), name
        gold[name + "/loss32"], gold[name + "/d_cls32"], gold[name + "/d_box32"] = o32.astype(F), c32, b32
        if c["dir"]:
            gold[name + "/d_dir32"] = d32
        assert np.array_equal(d["labels"], gold[name + "/labels"].astype(np.int32)), "the reference wrote the caller's labels"
        worst = 0.0
        if with_f64:
            o64, c64, b64, d64 = ref_loss(head, d, torch.float64)
            gold[name + "/loss64"], gold[name + "/d_cls64"], gold[name + "/d_box64"] = o64, c64, b64
            if c["dir"]:
                gold[name + "/d_dir64"] = d64
            # the restatement against the reference's float64 record, here where both run
            R = al.restate(d, own=True)
            for got, ref in ((R["out"], o64), (R["d_cls"], c64), (R["d_box"], b64)) + (((R["d_dir"], d64),) if c["dir"] else ()):
                err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
                assert np.isfinite(ref).all() and np.isfinite(got).all(), name
                worst = max(worst, float(np.where(ref == 0, np.where(got == 0, 0.0, np.inf), err).max()))
            assert worst < 1e-12, (name, worst)
        print("%-22s B %d A %3d C %d dir %-5s positives %-12s ignored %3d  f64 %-5s restatement vs f64 record %.1e  loss %s" %
              (name, d["labels"].shape[0], anchors.shape[0], d["cls"].shape[2], c["dir"], list(counts), int((d["labels"] < 0).sum()), with_f64, worst,
               np.round(o32, 5)))
        index.append(dict(name=name, map=c["map"], dir=c["dir"], f64=with_f64, clamp=bool(c.get("clamp")),
                          on_clamp=[int(v) for v in np.argwhere(on_clamp)[0]] if on_clamp is not None else None))
    gold["cases"] = np.array(json.dumps(index))
    path = os.path.join(HERE, "anchor_loss.npz")
    np.savez_compressed(path, **gold)
    print("wrote anchor_loss.npz %.0f KB" % (os.path.getsize(path) / 1024))
