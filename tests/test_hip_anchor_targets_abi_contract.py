"""The buffer contract of btc_anchor_targets and btc_decode_anchor_boxes (include/btcdet_hip_heads.h), as the other contract files hold
their entry points to it: every output is a Guarded buffer (poisoned payload between two guard bands) with spare entries past its
extent, the workspace is garbage (both patterns), the call runs on a side stream.  Afterwards the stated extent is fully overwritten and
equals the numpy restatement, nothing past it and no guard is touched, the inputs hold the bits they held, and the same call on the
current stream with another dirty workspace gives the same bits.  Refused arguments return -1, write nothing and enqueue nothing."""
import numpy as np
import pytest
import torch

import abi_contract as ac
import anchor_targets_ref as ar
import test_hip_anchor_targets as T

pytestmark = pytest.mark.gpu
SPARE = 5
EXACT = list(ar.EXACT)


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _inputs(grid, M):
    cfg, names, anchors, gt, want = T.edge_case(grid, M)
    flat = torch.cat(anchors, dim=-3).reshape(-1, 7).contiguous()
    return ar.host_tables(cfg, names), {"anchors": flat, "gt": _dev(gt)}, want


def _args(tables, t, A, B, M, labels, targets, weights, ws, ws_bytes):
    slot_cfg, matched, unmatched, class_cfg = tables
    return (t["anchors"].data_ptr() if A else None, A, int(slot_cfg.shape[0]), slot_cfg.ctypes.data, int(matched.shape[0]), matched.ctypes.data,
            unmatched.ctypes.data, class_cfg.ctypes.data, int(class_cfg.shape[0]) - 1, t["gt"].data_ptr() if M else None, B, M, labels, targets, weights,
            ws, ws_bytes)


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("case", [("A0", 1), ("A257", 0), ("A513", 65), ("A1530", 64)], ids=lambda c: "%s-M%d" % c)
def test_anchor_targets_buffer_contract(case, garbage):
    from btcdet_amd._lib import check, stream_ptr
    grid, M = case
    tables, t, want = _inputs(grid, M)
    A, B = int(t["anchors"].shape[0]), 3
    before = {k: v.clone() for k, v in t.items()}
    host_before = [a.copy() for a in tables]
    ws_bytes = L().btc_anchor_targets_ws_bytes(B, M)
    assert ws_bytes > 0
    ws = ac.Workspace(ws_bytes, garbage=garbage)
    n = B * A
    labels, targets, weights = ac.Guarded((n + SPARE,), "int32"), ac.Guarded((n + SPARE, 7), "float32"), ac.Guarded((n + SPARE,), "float32")
    ac.call("btc_anchor_targets", *_args(tables, t, A, B, M, labels.ptr, targets.ptr, weights.ptr, ws.ptr, ws_bytes))
    for g in (labels, targets, weights):
        assert not bool(g.poison_mask()[:n].any()) and bool(g.poison_mask()[n:].all()) and g.guards_intact()
    assert ws.guards_intact()
    got_l, got_t, got_w = labels.tensor[:n].cpu().numpy().reshape(B, A), targets.tensor[:n].cpu().numpy().reshape(B, A, 7), weights.tensor[:n].cpu().numpy().reshape(B, A)
    print(grid, "M", M, "positives", int((got_l > 0).sum()), "ignored", int((got_l < 0).sum()))
    assert np.array_equal(got_l, want[0]) and np.array_equal(got_w, want[2]) and np.array_equal(got_t[..., EXACT], want[1][..., EXACT])
    np.testing.assert_allclose(got_t, want[1], rtol=1e-5, atol=1e-6)
    for k, v in before.items():
        assert _same_bits(t[k], v), "input %s was written" % k
    for a, b in zip(tables, host_before):
        assert np.array_equal(a, b)
    # the same call on the current stream: ordinary buffers, another dirty workspace
    l2 = torch.full((n + SPARE,), 7, dtype=torch.int32, device="cuda")
    t2 = torch.full((n + SPARE, 7), 7.0, dtype=torch.float32, device="cuda")
    w2 = torch.full((n + SPARE,), 7.0, dtype=torch.float32, device="cuda")
    ws2 = torch.full((max(ws_bytes, 256),), 0x5A, dtype=torch.uint8, device="cuda")
    check(L().btc_anchor_targets(*_args(tables, t, A, B, M, l2.data_ptr(), t2.data_ptr(), w2.data_ptr(), ws2.data_ptr(), ws_bytes), stream_ptr()),
          "btc_anchor_targets")
    torch.cuda.synchronize()
    assert _same_bits(l2[:n], labels.tensor[:n]) and _same_bits(t2[:n], targets.tensor[:n]) and _same_bits(w2[:n], weights.tensor[:n])
    assert bool((l2[n:] == 7).all()) and bool((t2[n:] == 7).all()) and bool((w2[n:] == 7).all())


def test_anchor_targets_refusals_write_nothing():
    from btcdet_amd._lib import stream_ptr
    tables, t, _ = _inputs("A510", 65)
    A, B, M = int(t["anchors"].shape[0]), 3, 65
    ws = ac.Workspace(L().btc_anchor_targets_ws_bytes(B, M))
    labels, targets, weights = ac.Guarded((B * A,), "int32"), ac.Guarded((B * A, 7), "float32"), ac.Guarded((B * A,), "float32")
    good = list(_args(tables, t, A, B, M, labels.ptr, targets.ptr, weights.ptr, ws.ptr, ws.ws_bytes))
    names = ["anchors", "A", "slots", "slot_cfg", "ncfg", "matched", "unmatched", "class_cfg", "num_class", "gt", "B", "M", "labels", "targets", "weights",
             "ws", "ws_bytes"]
    bad_slot, bad_class = np.array([0, 1], np.int32), np.array([0, 1], np.int32)
    for kw in (dict(B=0), dict(B=-1), dict(A=-2), dict(M=-1), dict(slots=0), dict(slots=65), dict(A=A - 1), dict(ncfg=0), dict(ncfg=17), dict(num_class=-1),
               dict(num_class=64), dict(slot_cfg=bad_slot.ctypes.data), dict(class_cfg=bad_class.ctypes.data), dict(slot_cfg=None), dict(matched=None),
               dict(unmatched=None), dict(class_cfg=None), dict(anchors=None), dict(gt=None), dict(labels=None), dict(targets=None), dict(weights=None),
               dict(ws=None), dict(ws_bytes=ws.ws_bytes - 1), dict(ws_bytes=256), dict(ws_bytes=0)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert L().btc_anchor_targets(*a, stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    for g in (labels, targets, weights):
        assert bool(g.poison_mask().all()) and g.guards_intact()
    assert ws.guards_intact() and bool((ws.tensor == 0xA5).all()), "a refused call touched the workspace"
    # A == 0 is legal and launches nothing
    a = list(good)
    a[names.index("A")], a[names.index("anchors")] = 0, None
    assert L().btc_anchor_targets(*a, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(labels.poison_mask().all()) and bool((ws.tensor == 0xA5).all())


# ------------------------------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("bins", [0, 1, 2, 3], ids=lambda b: "bins%d" % b)
@pytest.mark.parametrize("A", [1, 255, 257, 513])
def test_decode_buffer_contract(A, bins):
    from btcdet_amd._lib import check, stream_ptr
    rng = np.random.default_rng(31 * A + bins)
    B, off, lim = 3, 0.78539, 0.0
    anchors = np.concatenate([rng.uniform(-20, 20, (A, 3)), rng.uniform(0.5, 4.0, (A, 3)), rng.choice([0.0, 1.57], (A, 1))], axis=1).astype(np.float32)
    preds = (rng.standard_normal((B, A, 7)) * 0.4).astype(np.float32)
    dirs = rng.standard_normal((B, A, bins)).astype(np.float32) if bins else None
    if bins:                                            # the generator's margins: no quotient near an integer, no tied logits
        q = (preds[..., 6].astype(np.float64) + anchors[None, :, 6] - off) / (2 * np.pi / bins) + lim
        preds[..., 6] += np.where(np.abs(q - np.round(q)) < 1e-3, np.float32(0.01), np.float32(0))
    ar.margins_decode(preds, anchors, dirs, off, lim, bins)
    want = ar.restate_decode(preds, anchors, dirs, off, lim, bins)
    t = {"preds": _dev(preds), "anchors": _dev(anchors)}
    if bins:
        t["dirs"] = _dev(dirs)
    before = {k: v.clone() for k, v in t.items()}
    n = B * A
    boxes = ac.Guarded((n + SPARE, 7), "float32")
    args = (t["preds"].data_ptr(), t["anchors"].data_ptr(), t["dirs"].data_ptr() if bins else None, B, A, bins, off, lim)
    ac.call("btc_decode_anchor_boxes", *args, boxes.ptr)
    assert not bool(boxes.poison_mask()[:n].any()) and bool(boxes.poison_mask()[n:].all()) and boxes.guards_intact()
    got = boxes.tensor[:n].cpu().numpy().reshape(B, A, 7)
    diff = np.abs(got.astype(np.float64) - want)
    print("A", A, "bins", bins, "max |diff| exact columns %.3e, exp columns %.3e" % (diff[..., EXACT].max(), diff[..., [3, 4, 5]].max()))
    assert np.array_equal(got[..., EXACT], want[..., EXACT])
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
    for k, v in before.items():
        assert _same_bits(t[k], v), "input %s was written" % k
    b2 = torch.full((n + SPARE, 7), 7.0, dtype=torch.float32, device="cuda")
    check(L().btc_decode_anchor_boxes(*args, b2.data_ptr(), stream_ptr()), "btc_decode_anchor_boxes")
    torch.cuda.synchronize()
    assert _same_bits(b2[:n], boxes.tensor[:n]) and bool((b2[n:] == 7).all())


def test_decode_refusals_write_nothing():
    from btcdet_amd._lib import stream_ptr
    B, A, bins = 2, 300, 2
    t = {"preds": torch.zeros((B, A, 7), device="cuda"), "anchors": torch.ones((A, 7), device="cuda"), "dirs": torch.zeros((B, A, bins), device="cuda")}
    boxes = ac.Guarded((B * A, 7), "float32")
    good = [t["preds"].data_ptr(), t["anchors"].data_ptr(), t["dirs"].data_ptr(), B, A, bins, 0.78539, 0.0, boxes.ptr]
    names = ["preds", "anchors", "dirs", "B", "A", "bins", "off", "lim", "boxes"]
    for kw in (dict(B=0), dict(B=-1), dict(A=-1), dict(preds=None), dict(anchors=None), dict(boxes=None), dict(bins=0), dict(bins=-1), dict(B=2 ** 16, A=2 ** 13)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert L().btc_decode_anchor_boxes(*a, stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    assert bool(boxes.poison_mask().all()) and boxes.guards_intact()
    a = list(good)
    a[names.index("A")] = 0
    assert L().btc_decode_anchor_boxes(*a, stream_ptr()) == 0          # A == 0 is legal and launches nothing
    torch.cuda.synchronize()
    assert bool(boxes.poison_mask().all())
