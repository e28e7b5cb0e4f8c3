"""The buffer contract of btc_occ_metrics (include/btcdet_hip_infer.h), as tests/test_hip_det_post_abi_contract.py holds the detections'
entry points to it: the output row is a Guarded buffer (poisoned payload between two guard bands), the workspace is garbage (both
patterns).  After a call the 16 counters are fully overwritten and equal the restatement, the guards are intact, the inputs hold the bits
they held, and the same call on the current stream gives the same bits.  Refused arguments write nothing."""
import numpy as np
import pytest
import torch

import abi_contract as ac
import occ_metrics_ref as ref

pytestmark = pytest.mark.gpu


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _g(a):
    return torch.from_numpy(np.array(a)).cuda()


def _inputs(n, M):
    B = 2
    num = [M, max(M - 3, 0)]
    bd = ref.seeded_case(seed=300 + n + M, shape=(B, 3, 5, 7), M=M, num=num, pts=[n - n // 2, n // 2], inside=0.7)
    t = {"prob": _g(bd["batch_pred_occ_prob"]), "cls": _g(bd["general_cls_loss_mask"]), "pos": _g(bd["pos_mask"]), "neg": _g(bd["neg_mask"]),
         "pos_all": torch.tensor([bd["pos_all_num"]], dtype=torch.int32, device="cuda"), "pnts": _g(bd["occ_pnts"]), "bind": _g(bd["added_occ_b_ind"]),
         "gt": _g(bd["gt_boxes"]), "gtn": torch.tensor(num, dtype=torch.int32, device="cuda")}
    return bd, t, B


def _args(t, n_cells, n, B, M, out_ptr, ws_ptr, ws_bytes):
    from btcdet_amd._lib import ptr
    return (ptr(t["prob"]), ptr(t["cls"]), ptr(t["pos"]), ptr(t["neg"]), n_cells, ptr(t["pos_all"]), ptr(t["pnts"]), ptr(t["bind"]), n, ptr(t["gt"]),
            ptr(t["gtn"]), B, M, 8, out_ptr, ws_ptr, ws_bytes)


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("n,M", [(1, 1), (65, 1), (4096, 1), (1, 65), (65, 65), (4096, 65)])
def test_occ_metrics_buffer_contract(n, M, garbage):
    from btcdet_amd._lib import check, ptr, stream_ptr
    bd, t, B = _inputs(n, M)
    before = {k: v.clone() for k, v in t.items()}
    n_cells = t["prob"].numel()
    ws_bytes = L().btc_occ_metrics_ws_bytes(B, M)
    ws = ac.Workspace(ws_bytes, garbage=garbage)
    out = ac.Guarded((16,), "int64")
    s = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    rc = L().btc_occ_metrics(*_args(t, n_cells, n, B, M, out.ptr, ws.ptr, ws_bytes), s.cuda_stream)
    s.synchronize()
    assert rc == 0, "rc %d: %s" % (rc, L().btc_last_error().decode("utf-8", "replace"))
    assert not bool(out.poison_mask().any()), "%d of 16 counters left as poison" % int(out.poison_mask().sum())
    assert out.guards_intact() and ws.guards_intact()
    got = out.tensor.cpu().numpy()
    want = ref.counters(bd)
    print("n", n, "M", M, "got", got.tolist(), "want", want.tolist())
    assert got.tolist() == want.tolist()
    for k, v in before.items():
        assert torch.equal(t[k].reshape(-1).view(torch.uint8), v.reshape(-1).view(torch.uint8)), "input %s was written" % k
    # the same call on the current stream (an ordinary output and workspace, no guards) gives the same bits
    again = torch.empty((16,), dtype=torch.int64, device="cuda")
    w2 = torch.empty((max(ws_bytes, 256),), dtype=torch.uint8, device="cuda")
    check(L().btc_occ_metrics(*_args(t, n_cells, n, B, M, ptr(again), ptr(w2), ws_bytes), stream_ptr()), "btc_occ_metrics")
    torch.cuda.synchronize()
    assert torch.equal(again, out.tensor)


def test_nothing_is_written_when_the_arguments_are_refused():
    from btcdet_amd._lib import ptr, stream_ptr
    n, M = 65, 5
    bd, t, B = _inputs(n, M)
    n_cells = t["prob"].numel()
    ws = ac.Workspace(L().btc_occ_metrics_ws_bytes(B, M))
    out = ac.Guarded((16,), "int64")
    base = dict(prob=ptr(t["prob"]), cls=ptr(t["cls"]), pos=ptr(t["pos"]), neg=ptr(t["neg"]), n_cells=n_cells, pos_all=ptr(t["pos_all"]),
                pnts=ptr(t["pnts"]), bind=ptr(t["bind"]), n=n, gt=ptr(t["gt"]), gtn=ptr(t["gtn"]), B=B, M=M, stride=8, out=out.ptr, ws=ws.ptr,
                ws_bytes=ws.ws_bytes)
    order = ["prob", "cls", "pos", "neg", "n_cells", "pos_all", "pnts", "bind", "n", "gt", "gtn", "B", "M", "stride", "out", "ws", "ws_bytes"]
    for kw in (dict(n_cells=-1), dict(n=-1), dict(B=-1), dict(M=-1), dict(prob=None), dict(cls=None), dict(pos=None), dict(neg=None), dict(pos_all=None),
               dict(pnts=None), dict(bind=None), dict(gt=None), dict(gtn=None), dict(stride=6), dict(ws_bytes=ws.ws_bytes - 1), dict(ws_bytes=8)):
        a = dict(base, **kw)
        rc = L().btc_occ_metrics(*[a[k] for k in order], stream_ptr())
        assert rc == -1, kw
    torch.cuda.synchronize()
    assert bool(out.poison_mask().all()) and out.guards_intact()
    assert ws.guards_intact() and bool((ws.tensor == 0xA5).all())
