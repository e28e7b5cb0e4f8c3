"""The buffer contract of btc_fov_crop (include/btcdet_hip_frames.h), as the other contract files hold their entry points to it: out,
out_offsets and keep_idx are Guarded buffers (poisoned payload between two guard bands) with spare rows past n, the workspace is garbage
(both patterns), the call runs on a side stream.  Afterwards rows [0, n') of out and keep_idx are fully overwritten and equal the numpy
restatement, rows past n' and the guards are untouched, out_offsets[0..batch] is written and nothing past it, the inputs hold the bits
they held, and the same call on the current stream gives the same bits.  Refused arguments write nothing and enqueue nothing."""
import numpy as np
import pytest
import torch

import abi_contract as ac
import kitti_frames_ref as kr
import test_hip_fov_crop as T

pytestmark = pytest.mark.gpu
SPARE = 5          # rows of capacity beyond n: there is always a row past n'


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _device(pts, offs, blocks):
    return {"pts": torch.from_numpy(np.ascontiguousarray(pts)).cuda(), "offs": torch.from_numpy(np.asarray(offs, np.int32)).cuda(),
            "cal": torch.from_numpy(np.stack(blocks)).cuda()}


def _args(t, n, ld, B, cap, out, out_offs, idx, ws, ws_bytes):
    return (t["pts"].data_ptr() if n else None, n, ld, t["offs"].data_ptr(), B, t["cal"].data_ptr(), cap, out, out_offs, idx, ws, ws_bytes)


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("ld", [4, 5])
@pytest.mark.parametrize("sizes", [(0,), (1, 0), (257, 0, 130), (20,) * 9 + (400,)], ids=["0", "1", "387", "580"])
def test_fov_crop_buffer_contract(sizes, ld, garbage):
    from btcdet_amd._lib import check, stream_ptr
    pts, offs, blocks = T.batch(sizes, ld=ld, seed=3)
    n, B = pts.shape[0], len(sizes)
    want, want_offs, want_idx = kr.restate_crop(pts, offs, blocks)
    total = int(want_offs[-1])
    t = _device(pts, offs, blocks)
    before = {k: v.clone() for k, v in t.items()}
    cap = n + SPARE
    ws_bytes = L().btc_fov_crop_ws_bytes(n, B)
    ws = ac.Workspace(ws_bytes, garbage=garbage)
    out, idx = ac.Guarded((cap, ld), "float32"), ac.Guarded((cap,), "int32")
    out_offs = ac.Guarded((B + 1 + SPARE,), "int32")               # spare entries: nothing is written past out_offsets[batch]
    ac.call("btc_fov_crop", *_args(t, n, ld, B, cap, out.ptr, out_offs.ptr, idx.ptr, ws.ptr, ws_bytes))
    print("rows", list(sizes), "ld", ld, "kept", np.diff(want_offs).tolist())
    assert not bool(out_offs.poison_mask()[:B + 1].any()) and bool(out_offs.poison_mask()[B + 1:].all())
    assert out_offs.tensor[:B + 1].cpu().tolist() == want_offs.tolist()
    assert not bool(out.poison_mask()[:total].any()), "a row below n' was left unwritten"
    assert bool(out.poison_mask()[total:].all()), "a row past n' was written"
    assert not bool(idx.poison_mask()[:total].any()) and bool(idx.poison_mask()[total:].all())
    assert out.tensor[:total].cpu().numpy().tobytes() == want.tobytes() and idx.tensor[:total].cpu().tolist() == want_idx.tolist()
    assert out.guards_intact() and idx.guards_intact() and out_offs.guards_intact() and ws.guards_intact()
    for k, v in before.items():
        assert torch.equal(t[k].reshape(-1).view(torch.uint8), v.reshape(-1).view(torch.uint8)), "input %s was written" % k
    # the same call on the current stream (ordinary buffers, no guards, another dirty workspace, no keep_idx) gives the same bits
    o2 = torch.zeros((cap, ld), device="cuda")
    f2 = torch.zeros((B + 1,), dtype=torch.int32, device="cuda")
    w2 = torch.full((max(ws_bytes, 256),), 0x5A, dtype=torch.uint8, device="cuda")
    check(L().btc_fov_crop(*_args(t, n, ld, B, cap, o2.data_ptr(), f2.data_ptr(), None, w2.data_ptr(), ws_bytes), stream_ptr()), "btc_fov_crop")
    torch.cuda.synchronize()
    assert torch.equal(f2, out_offs.tensor[:B + 1])
    assert torch.equal(o2[:total].view(torch.int32), out.tensor[:total].view(torch.int32)) and not bool(o2[total:].any())


def test_nothing_is_written_when_the_arguments_are_refused():
    from btcdet_amd._lib import stream_ptr
    sizes, ld = (257, 0, 130), 4
    pts, offs, blocks = T.batch(sizes, ld=ld, seed=3)
    n, B = pts.shape[0], len(sizes)
    t = _device(pts, offs, blocks)
    cap = n + SPARE
    ws = ac.Workspace(L().btc_fov_crop_ws_bytes(n, B))
    out, idx, out_offs = ac.Guarded((cap, ld), "float32"), ac.Guarded((cap,), "int32"), ac.Guarded((B + 1,), "int32")
    good = list(_args(t, n, ld, B, cap, out.ptr, out_offs.ptr, idx.ptr, ws.ptr, ws.ws_bytes))
    names = ["pts", "n", "ld", "offs", "batch", "cal", "cap", "out", "out_offs", "idx", "ws", "ws_bytes"]
    for kw in (dict(ld=2), dict(ld=0), dict(batch=0), dict(batch=-1), dict(n=-1), dict(cap=n - 1), dict(cap=0), dict(pts=None), dict(offs=None),
               dict(cal=None), dict(out=None), dict(out_offs=None), dict(ws=None), dict(ws_bytes=ws.ws_bytes - 1), dict(ws_bytes=8), dict(ws_bytes=0)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert L().btc_fov_crop(*a, stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    for g in (out, idx, out_offs):
        assert bool(g.poison_mask().all()) and g.guards_intact()
    assert ws.guards_intact() and bool((ws.tensor == 0xA5).all()), "a refused call touched the workspace"
