"""The buffer contract of btc_roi_loss_fwd and btc_roi_loss_bwd (include/btcdet_hip_roi_loss.h), as the other contract files hold their
entry points to it: every output is a Guarded buffer (poisoned payload between two guard bands) with spare entries past its extent, the
workspace is garbage past its 256-byte zero head (both patterns) and the head is left zero, the calls run on a side stream.  Afterwards
the stated extent is fully overwritten and lies inside the derived bound of tests/roi_loss_ref.py, nothing past it and no guard is
touched, and the inputs hold the bits they held.  Refused arguments return -1, write nothing and enqueue nothing."""
import numpy as np
import pytest
import torch

import abi_contract as ac
import roi_loss_ref as rl

pytestmark = pytest.mark.gpu
SPARE = 5


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return a.numel() == b.numel() == 0 or torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _inputs(case):
    d = rl.make_case(case)
    return d, {k: _dev(d[k]) for k in ("cls", "reg", "rois", "gt", "src", "mask", "labels")}


def _args(d, t):
    N = d["mask"].size
    p = lambda k: t[k].data_ptr() if N else None
    w = d["w"]
    return [p("cls"), p("reg"), p("rois"), p("gt"), p("src"), 8, p("mask"), p("labels"), rl.kind_of(d), N, int(d["corner"]), w["rcnn_cls_weight"],
            w["rcnn_reg_weight"], w["rcnn_corner_weight"]]


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("case", [dict(N=0, kind="random", labels="roi_iou", corner=True), dict(N=2 * rl.TILE + 3, kind="random", labels="cls", corner=True),
                                  dict(N=rl.VALUE_N, kind="nan_target", labels="roi_iou", corner=False)], ids=rl.case_name)
def test_roi_loss_buffer_contract(case, garbage):
    d, t = _inputs(case)
    N = d["mask"].size
    before = {k: v.clone() for k, v in t.items()}
    ws_bytes = L().btc_roi_loss_ws_bytes(N)
    assert ws_bytes >= 256 + 40
    ws = ac.Workspace(ws_bytes, zero_head=256, garbage=garbage)
    out, norms = ac.Guarded((5 + SPARE,), "float32"), ac.Guarded((2 + SPARE,), "float32")
    ac.call("btc_roi_loss_fwd", *_args(d, t), out.ptr, norms.ptr, ws.ptr, ws_bytes)
    assert ws.head_zero() and ws.guards_intact() and bool((ws.tensor[256 + min(max(-(-N // rl.TILE), 1), rl.MAX_TILES) * 40:] == garbage).all())
    for gd, ext in ((out, 5), (norms, 2)):
        assert not bool(gd.poison_mask()[:ext].any()) and bool(gd.poison_mask()[ext:].all()) and gd.guards_intact()
    d_cls, d_reg = ac.Guarded((N + SPARE,), "float32"), ac.Guarded((N + SPARE, 7), "float32")
    gup = torch.tensor([rl.G_UP], dtype=torch.float32, device="cuda")
    ac.call("btc_roi_loss_bwd", *_args(d, t), norms.ptr, gup.data_ptr(), d_cls.ptr if N else None, d_reg.ptr if N else None)
    for gd in (d_cls, d_reg):
        assert not bool(gd.poison_mask()[:N].any()) and bool(gd.poison_mask()[N:].all()) and gd.guards_intact()
    for k, v in before.items():
        assert _same_bits(t[k], v), "input %s was written" % k
    got = dict(out=out.tensor[:5].cpu().numpy(), norms=norms.tensor[:2].cpu().numpy(), d_cls=d_cls.tensor[:N].cpu().numpy(), d_reg=d_reg.tensor[:N].cpu().numpy(),
               g=rl.G_UP)
    W = rl.Worst()
    rl.check_roi(W, d, got, rl.case_name(case))
    print(rl.case_name(case), W.report())
    if N == 0:
        assert np.array_equal(got["out"], np.zeros(5, np.float32)) and np.array_equal(got["norms"], np.ones(2, np.float32))


def test_roi_loss_refusals_write_nothing():
    from btcdet_amd._lib import stream_ptr
    d, t = _inputs(dict(N=300, kind="random", labels="roi_iou", corner=True))
    N = 300
    ws = ac.Workspace(L().btc_roi_loss_ws_bytes(N), zero_head=256)
    out, norms = ac.Guarded((5,), "float32"), ac.Guarded((2,), "float32")
    d_cls, d_reg = ac.Guarded((N,), "float32"), ac.Guarded((N, 7), "float32")
    gup = torch.ones(1, device="cuda")
    ones = torch.ones(2, device="cuda")
    names = ["cls", "reg", "rois", "gt", "src", "gt_width", "mask", "labels", "kind", "N", "corner", "cw", "rw", "kw"]
    fwd = dict(zip(names, _args(d, t)), out=out.ptr, norms=norms.ptr, ws=ws.ptr, ws_bytes=ws.ws_bytes)
    bwd = dict(zip(names, _args(d, t)), norms=ones.data_ptr(), grad=gup.data_ptr(), d_cls=d_cls.ptr, d_reg=d_reg.ptr)
    common = [dict(N=-1), dict(N=2 ** 28), dict(gt_width=6), dict(gt_width=0), dict(kind=2), dict(kind=-1), dict(cls=None), dict(reg=None), dict(rois=None),
              dict(gt=None), dict(src=None), dict(mask=None), dict(labels=None)]
    for fn, good, extra in ((L().btc_roi_loss_fwd, fwd, [dict(out=None), dict(norms=None), dict(ws=None), dict(ws_bytes=ws.ws_bytes - 1), dict(ws_bytes=256)]),
                            (L().btc_roi_loss_bwd, bwd, [dict(norms=None), dict(grad=None), dict(d_cls=None), dict(d_reg=None)])):
        for kw in common + extra:
            assert fn(*dict(good, **kw).values(), stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    for gd in (out, norms, d_cls, d_reg):
        assert bool(gd.poison_mask().all()) and gd.guards_intact()
    assert ws.guards_intact() and ws.head_zero() and bool((ws.tensor[256:] == 0xA5).all()), "a refused call touched the workspace"
