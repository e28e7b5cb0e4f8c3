"""The buffer contract of btc_anchor_loss_fwd and btc_anchor_loss_bwd (include/btcdet_hip_anchor_loss.h), as the other contract files hold
their entry points to it: every output is a Guarded buffer (poisoned payload between two guard bands) with spare entries past its
extent, the workspace is garbage past its 256-byte zero head (both patterns) and the head is left zero, the calls run on a side stream.
Afterwards the stated extent is fully overwritten and lies inside the derived bound of tests/anchor_loss_ref.py, nothing past it and no
guard is touched, and the inputs -- the labels included -- hold the bits they held.  Refused arguments return -1, write nothing and
enqueue nothing."""
import numpy as np
import pytest
import torch

import abi_contract as ac
import anchor_loss_ref as al

pytestmark = pytest.mark.gpu
SPARE = 5


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _inputs(case):
    d = al.make_case(case)
    t = {k: _dev(d[k]) for k in ("cls", "box", "labels", "tgt", "anchors")}
    if d["dir"] is not None:
        t["dir"] = _dev(d["dir"])
    return d, t


def _args(d, t):
    B, A, C = d["cls"].shape
    bins = 0 if d["dir"] is None else d["dir"].shape[2]
    p = lambda k: t[k].data_ptr() if (k in t and A) else None
    w = d["w"]
    return [p("cls"), p("box"), p("dir"), p("labels"), p("tgt"), p("anchors"), B, A, C, bins, w["cls_weight"], w["loc_weight"], w["dir_weight"] if bins else 0.0,
            d["dir_offset"]]


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("case", [dict(B=1, A=0, C=1, bins=2, kind="random"), dict(B=3, A=257, C=3, bins=2, kind="random"),
                                  dict(B=2, A=513, C=1, bins=0, kind="nan_target")], ids=al.case_name)
def test_anchor_loss_buffer_contract(case, garbage):
    d, t = _inputs(case)
    B, A, C = d["cls"].shape
    bins = 0 if d["dir"] is None else d["dir"].shape[2]
    before = {k: v.clone() for k, v in t.items()}
    ws_bytes = L().btc_anchor_loss_ws_bytes(B, A)
    assert ws_bytes >= 256 + 32
    ws = ac.Workspace(ws_bytes, zero_head=256, garbage=garbage)
    n = B * A
    out, norms = ac.Guarded((4 + SPARE,), "float32"), ac.Guarded((B + SPARE,), "float32")
    ac.call("btc_anchor_loss_fwd", *_args(d, t), out.ptr, norms.ptr, ws.ptr, ws_bytes)
    assert ws.head_zero() and ws.guards_intact() and bool((ws.tensor[256 + B * min(max(-(-A // al.THREADS), 1), al.MAX_TILES) * 32:] == garbage).all())
    for gd, ext in ((out, 4), (norms, B)):
        assert not bool(gd.poison_mask()[:ext].any()) and bool(gd.poison_mask()[ext:].all()) and gd.guards_intact()
    d_cls, d_box, d_dir = ac.Guarded((n + SPARE, C), "float32"), ac.Guarded((n + SPARE, 7), "float32"), ac.Guarded((n + SPARE, max(bins, 1)), "float32")
    gup = torch.tensor([al.G_UP], dtype=torch.float32, device="cuda")
    ac.call("btc_anchor_loss_bwd", *_args(d, t), norms.ptr, gup.data_ptr(), d_cls.ptr if A else None, d_box.ptr if A else None, d_dir.ptr if (A and bins) else None)
    for gd in (d_cls, d_box) + ((d_dir,) if bins else ()):
        assert not bool(gd.poison_mask()[:n].any()) and bool(gd.poison_mask()[n:].all()) and gd.guards_intact()
    assert bins or bool(d_dir.poison_mask().all())
    for k, v in before.items():
        assert _same_bits(t[k], v), "input %s was written" % k
    got = dict(out=out.tensor[:4].cpu().numpy(), norms=norms.tensor[:B].cpu().numpy(), d_cls=d_cls.tensor[:n].cpu().numpy().reshape(B, A, C),
               d_box=d_box.tensor[:n].cpu().numpy().reshape(B, A, 7), d_dir=d_dir.tensor[:n].cpu().numpy().reshape(B, A, bins) if bins else None, g=al.G_UP)
    W = al.Worst()
    al.check_anchor(W, d, got, al.case_name(case))
    print(al.case_name(case), W.report())
    if A == 0:
        assert np.array_equal(got["out"], np.zeros(4, np.float32)) and np.array_equal(got["norms"], np.ones(B, np.float32))


def test_anchor_loss_refusals_write_nothing():
    from btcdet_amd._lib import stream_ptr
    d, t = _inputs(dict(B=2, A=300, C=3, bins=2, kind="random"))
    B, A, C, bins = 2, 300, 3, 2
    ws = ac.Workspace(L().btc_anchor_loss_ws_bytes(B, A), zero_head=256)
    out, norms = ac.Guarded((4,), "float32"), ac.Guarded((B,), "float32")
    d_cls, d_box, d_dir = ac.Guarded((B * A, C), "float32"), ac.Guarded((B * A, 7), "float32"), ac.Guarded((B * A, bins), "float32")
    gup = torch.ones(1, device="cuda")
    ones = torch.ones(B, device="cuda")
    names = ["cls", "box", "dir", "labels", "tgt", "anchors", "B", "A", "C", "bins", "cw", "lw", "dw", "off"]
    fwd = dict(zip(names, _args(d, t)), out=out.ptr, norms=norms.ptr, ws=ws.ptr, ws_bytes=ws.ws_bytes)
    bwd = dict(zip(names, _args(d, t)), norms=ones.data_ptr(), grad=gup.data_ptr(), d_cls=d_cls.ptr, d_box=d_box.ptr, d_dir=d_dir.ptr)
    common = [dict(B=0), dict(B=-1), dict(A=-1), dict(C=0), dict(C=64), dict(bins=-1), dict(bins=17), dict(cls=None), dict(box=None), dict(dir=None),
              dict(labels=None), dict(tgt=None), dict(anchors=None), dict(B=2 ** 12, A=2 ** 17)]
    for fn, good, extra in ((L().btc_anchor_loss_fwd, fwd, [dict(out=None), dict(norms=None), dict(ws=None), dict(ws_bytes=ws.ws_bytes - 1), dict(ws_bytes=256)]),
                            (L().btc_anchor_loss_bwd, bwd, [dict(norms=None), dict(grad=None), dict(d_cls=None), dict(d_box=None), dict(d_dir=None)])):
        for kw in common + extra:
            assert fn(*dict(good, **kw).values(), stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    for gd in (out, norms, d_cls, d_box, d_dir):
        assert bool(gd.poison_mask().all()) and gd.guards_intact()
    assert ws.guards_intact() and ws.head_zero() and bool((ws.tensor[256:] == 0xA5).all()), "a refused call touched the workspace"
