#!/usr/bin/env python3
"""ROI-head loss: the torch formulation of ConvHead.get_loss() against the fused calls, alternating in ONE process.

KITTI-Car ROI head (ROI_PER_IMAGE 128, batch size 2: N = 256 sampled rois), targets from DeviceProposalTargets over the proposals of
tools/roi_targets_bench.py (thirds of foreground / hard / easy proposals around the boxes of synth.make_scene).  Two ConvHead of the same
configuration that only compute their loss, one without ROI_HEAD.LOSS_CONFIG.DEVICE (`torch`: THE BASELINE -- rcnn_cls_loss /
rcnn_reg_loss of btcdet_amd/roi_targets.py, the code of the parent commit) and one with it (`fused`: btcdet_amd/roi_loss.py).

What is timed: get_loss() plus backward() to rcnn_cls and rcnn_reg (leaves; their .grad is dropped between calls).  Host clock around
--calls calls ending in a device synchronisation, `torch` and `fused` alternating --alternations times; per route the median block, and
the spread (max - min) of the blocks.  Kernel launches per call are counted as tools/anchor_targets_bench.py counts them.  --lib loads
another build of the library (one compiled with -DBTC_ROI_LOSS_LANES=8: a lane per corner); --compare-lib times the two launches alone,
by device events, on the loaded build and on another one, alternating in the same process.  Not measured here: the effect on a
--heads full training step (the step has its own bench).
Writes profiles/roi_loss_bench.json.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--batches", type=int, default=4, help="distinct target batches, cycled")
    ap.add_argument("--alternations", type=int, default=5, help="timed blocks PER ROUTE (at least 5 for a result that is reported)")
    ap.add_argument("--calls", type=int, default=500, help="calls per timed block")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lib", default=None, help="load this libbtcdet_hip.so instead of the package's (a build with other tile constants)")
    ap.add_argument("--compare-lib", default=None, help="also time the two launches alone, by device events, on the loaded library and on this one, alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_loss_bench.json"))
    return ap.parse_args(argv)


def loss_head(device_key):
    """a ConvHead that only computes its loss, with the shipped ROI_HEAD configuration"""
    import torch
    from btcdet_amd.config import load_cfg
    from btcdet_amd.conv_head import ConvHead
    from btcdet_amd.dense_head import ResidualCoder
    cfg = copy.deepcopy(load_cfg().MODEL.ROI_HEAD)
    if device_key:
        cfg.LOSS_CONFIG["DEVICE"] = True
    head = ConvHead.__new__(ConvHead)
    torch.nn.Module.__init__(head)
    head.model_cfg, head.box_coder = cfg, ResidualCoder()
    return head


def measure(args, device):
    import torch
    from anchor_targets_bench import launches
    from btcdet_amd.config import load_cfg
    from btcdet_amd.roi_targets_device import DeviceProposalTargets
    from roi_targets_bench import make_batch
    roi_head = load_cfg().MODEL.ROI_HEAD
    B = args.batch_size
    n_prop = int(roi_head.NMS_CONFIG["TRAIN"]["NMS_POST_MAXSIZE"])
    assign = DeviceProposalTargets(roi_head.TARGET_CONFIG)
    targets = [assign(make_batch(B, n_prop, s, device)) for s in range(args.batches)]
    N = int(targets[0]["reg_valid_mask"].numel())
    heads = {"torch": loss_head(False), "fused": loss_head(True)}
    torch.manual_seed(0)
    preds = dict(rcnn_cls=(torch.randn(N, 1, device=device) * 2.0).requires_grad_(True), rcnn_reg=(torch.randn(N, 7, device=device) * 0.2).requires_grad_(True))

    def fn(route):
        h = heads[route]

        def call(i=0):
            h.forward_ret_dict = dict(targets[i % len(targets)], **preds)
            for p in preds.values():
                p.grad = None
            loss, tb = h.get_loss()
            loss.backward()
            return loss, tb
        return call

    routes = ["torch", "fused"]
    (la, ta), ga = fn("torch")(), {k: p.grad.clone() for k, p in preds.items()}
    (lb, tb), gb = fn("fused")(), {k: p.grad.clone() for k, p in preds.items()}
    assert heads["fused"].device_loss and not heads["torch"].device_loss
    res = {"batch_size": B, "rois": N, "library": args.lib or "package",
           "foreground_per_batch": [int((t["reg_valid_mask"] > 0).sum()) for t in targets], "calls_per_block": args.calls,
           "loss": {"torch": float(la), "fused": float(lb)}, "tb_keys_agree": list(ta) == list(tb),
           "grad_max_abs_diff": {k: float((ga[k] - gb[k]).abs().max()) for k in preds},
           "launches_per_call": {r: launches(fn(r)) for r in routes}, "us_per_call": {r: [] for r in routes}}

    def block(route, n):
        f = fn(route)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            f(i)
        torch.cuda.synchronize()      # inside the host clock
        return (time.perf_counter() - t0) / n * 1e6

    for r in routes:
        block(r, max(args.warmup, 10))
    for _ in range(args.alternations):
        for r in routes:
            res["us_per_call"][r].append(block(r, args.calls))
    res["us_per_call_median"] = {r: statistics.median(v) for r, v in res["us_per_call"].items()}
    res["us_per_call_spread"] = {r: max(v) - min(v) for r, v in res["us_per_call"].items()}
    med, spr = res["us_per_call_median"], res["us_per_call_spread"]
    res["fused_below_torch_by_more_than_torch_spread"] = bool(med["torch"] - med["fused"] > spr["torch"])
    return res


def kernels_alone(args, device, other):
    """btc_roi_loss_fwd + btc_roi_loss_bwd through ctypes on two builds of the library in one process: device events around --calls pairs,
    the builds alternating --alternations times -> us per pair (median, spread) of each"""
    import ctypes
    import torch
    from btcdet_amd import _lib
    from btcdet_amd.config import load_cfg
    from btcdet_amd.roi_targets_device import DeviceProposalTargets
    from roi_targets_bench import make_batch
    roi_head = load_cfg().MODEL.ROI_HEAD
    t = DeviceProposalTargets(roi_head.TARGET_CONFIG)(make_batch(args.batch_size, int(roi_head.NMS_CONFIG["TRAIN"]["NMS_POST_MAXSIZE"]), 0, device))
    N = int(t["reg_valid_mask"].numel())
    torch.manual_seed(0)
    cls, reg = torch.randn(N, 1, device=device) * 2.0, torch.randn(N, 7, device=device) * 0.2
    out, norms, g = torch.empty(5, device=device), torch.empty(2, device=device), torch.ones(1, device=device)
    d_cls, d_reg = torch.empty_like(cls), torch.empty_like(reg)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=device)
    libs = {"loaded": _lib.lib(), "other": ctypes.CDLL(os.path.abspath(other))}
    for name in ("btc_roi_loss_fwd", "btc_roi_loss_bwd", "btc_roi_loss_ws_bytes"):
        fn = getattr(libs["other"], name)
        fn.restype, fn.argtypes = _lib._ROI_LOSS_SIGS[name]
    p = lambda x: x.data_ptr()
    common = (p(cls), p(reg), p(t["rois"]), p(t["gt_of_rois"]), p(t["gt_of_rois_src"]), 8, p(t["reg_valid_mask"]), p(t["rcnn_cls_labels"]), 0, N, 1, 1.0, 1.0, 1.0)

    def pair(L):
        assert L.btc_roi_loss_fwd(*common, p(out), p(norms), p(ws), int(L.btc_roi_loss_ws_bytes(N)), None) == 0
        assert L.btc_roi_loss_bwd(*common, p(norms), p(g), p(d_cls), p(d_reg), None) == 0

    def block(L, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            pair(L)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3

    bits = {}
    for k, L in libs.items():
        block(L, 20)
        bits[k] = [x.clone() for x in (out, d_cls, d_reg)]
    us = {k: [] for k in libs}
    for _ in range(args.alternations):
        for k, L in libs.items():
            us[k].append(block(L, args.calls))
    # (the tile of each build, read off its workspace size: the first N that needs a second workgroup is TILE + 1)
    tile = {k: next(n for n in range(1, 1025) if int(L.btc_roi_loss_ws_bytes(n + 1)) > 256 + 40) for k, L in libs.items()}
    return {"other_library": other, "rois": N, "rois_per_workgroup": tile, "us_per_pair": us, "us_per_pair_median": {k: statistics.median(v) for k, v in us.items()},
            "us_per_pair_spread": {k: max(v) - min(v) for k, v in us.items()},
            "outputs_equal_bit_for_bit": bool(all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(bits["loaded"], bits["other"])))}


def main(argv=None):
    args = parse_args(argv)
    import torch
    import infer_bench
    if args.lib:
        from btcdet_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.lib)
        os.environ["BTC_FASTPATH"] = "0"      # the compiled binding belongs to the package's library
    assert torch.cuda.is_available(), "tools/roi_loss_bench.py needs a GPU"
    out = {"head": infer_bench.head_commit(), "alternations": args.alternations, "roi_loss": measure(args, torch.device("cuda:0"))}
    print(json.dumps(out["roi_loss"]), flush=True)
    if args.compare_lib:
        out["kernels_alone"] = kernels_alone(args, torch.device("cuda:0"), args.compare_lib)
        print(json.dumps(out["kernels_alone"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
