"""The buffer contract of btc_cut_objects (include/btcdet_hip_gtdb.h), as the other contract files hold their entry points to it: out,
obj_offsets and src_idx are Guarded buffers (poisoned payload between two guard bands) with spare rows past the total, the workspace is
garbage (both patterns), the call runs on a side stream.  Afterwards rows [0, total) of out and src_idx are fully overwritten and equal
the numpy restatement, rows past the total and the guards are untouched, obj_offsets[0..m] is written and nothing past it, the inputs
hold the bits they held, and the same call on the current stream gives the same bits.  Refused arguments write nothing and enqueue
nothing."""
import numpy as np
import pytest
import torch

import abi_contract as ac
import gt_database_ref as gr
import test_hip_gt_database as T

pytestmark = pytest.mark.gpu
SPARE = 5          # rows of capacity beyond the total, entries beyond obj_offsets[m]


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _device(pts, offs, boxes):
    from btcdet_amd.gt_database import cut_layout
    lay = cut_layout(offs, boxes)
    t = {"pts": torch.from_numpy(np.ascontiguousarray(pts)).cuda()}
    t.update({k: torch.from_numpy(np.ascontiguousarray(lay[k])).cuda() for k in ("rows", "centre", "box_offsets", "scene_offsets")})
    return t, lay


def _args(t, n, ld, B, m, max_boxes, cap, out, obj_offs, idx, ws, ws_bytes):
    return (t["pts"].data_ptr() if n else None, n, ld, t["scene_offsets"].data_ptr(), B, t["rows"].data_ptr() if m else None,
            t["centre"].data_ptr() if m else None, t["box_offsets"].data_ptr(), m, max_boxes, cap, out, obj_offs, idx, ws, ws_bytes)


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("ld", [4, 5])
@pytest.mark.parametrize("case", [((0,), (2,)), ((1, 0), (1, 0)), ((257, 0, 130), (3, 2, 0)), ((20,) * 9 + (400,), (1,) * 9 + (66,))],
                         ids=["0", "1", "387", "580"])
def test_cut_objects_buffer_contract(case, ld, garbage):
    from btcdet_amd._lib import check, stream_ptr
    sizes, nboxes = case
    pts, offs, boxes = T.make_batch(sizes, nboxes, ld=ld, seed=3)
    n, B = pts.shape[0], len(sizes)
    want, want_offs, want_idx = gr.restate_cut(pts, offs, boxes)
    total = int(want_offs[-1])
    t, lay = _device(pts, offs, boxes)
    m, max_boxes = lay["m"], lay["max_boxes"]
    before = {k: v.clone() for k, v in t.items()}
    cap = total + SPARE
    ws_bytes = L().btc_cut_objects_ws_bytes(n, B, m, max_boxes)
    ws = ac.Workspace(ws_bytes, garbage=garbage)
    out, idx = ac.Guarded((cap, ld), "float32"), ac.Guarded((cap,), "int32")
    obj_offs = ac.Guarded((m + 1 + SPARE,), "int32")               # spare entries: nothing is written past obj_offsets[m]
    ac.call("btc_cut_objects", *_args(t, n, ld, B, m, max_boxes, cap, out.ptr, obj_offs.ptr, idx.ptr, ws.ptr, ws_bytes))
    print("rows", list(sizes), "boxes", list(nboxes), "ld", ld, "total", total)
    assert not bool(obj_offs.poison_mask()[:m + 1].any()) and bool(obj_offs.poison_mask()[m + 1:].all())
    assert obj_offs.tensor[:m + 1].cpu().tolist() == want_offs.tolist()
    assert not bool(out.poison_mask()[:total].any()), "a row below the total was left unwritten"
    assert bool(out.poison_mask()[total:].all()), "a row past the total was written"
    assert not bool(idx.poison_mask()[:total].any()) and bool(idx.poison_mask()[total:].all())
    assert out.tensor[:total].cpu().numpy().tobytes() == want.tobytes() and idx.tensor[:total].cpu().tolist() == want_idx.tolist()
    assert out.guards_intact() and idx.guards_intact() and obj_offs.guards_intact() and ws.guards_intact()
    for k, v in before.items():
        assert torch.equal(t[k].reshape(-1).view(torch.uint8), v.reshape(-1).view(torch.uint8)), "input %s was written" % k
    # the same call on the current stream (ordinary buffers, no guards, another dirty workspace, no src_idx) gives the same bits
    o2 = torch.zeros((cap, ld), device="cuda")
    f2 = torch.zeros((m + 1,), dtype=torch.int32, device="cuda")
    w2 = torch.full((max(ws_bytes, 256),), 0x5A, dtype=torch.uint8, device="cuda")
    check(L().btc_cut_objects(*_args(t, n, ld, B, m, max_boxes, cap, o2.data_ptr(), f2.data_ptr(), None, w2.data_ptr(), ws_bytes), stream_ptr()),
          "btc_cut_objects")
    torch.cuda.synchronize()
    assert torch.equal(f2, obj_offs.tensor[:m + 1])
    assert torch.equal(o2[:total].view(torch.int32), out.tensor[:total].view(torch.int32)) and not bool(o2[total:].any())


def test_nothing_is_written_when_the_arguments_are_refused():
    from btcdet_amd._lib import stream_ptr
    sizes, nboxes, ld = (257, 0, 130), (3, 2, 1), 4
    pts, offs, boxes = T.make_batch(sizes, nboxes, ld=ld, seed=3)
    n, B = pts.shape[0], len(sizes)
    t, lay = _device(pts, offs, boxes)
    m, max_boxes = lay["m"], lay["max_boxes"]
    cap = n + SPARE
    ws = ac.Workspace(L().btc_cut_objects_ws_bytes(n, B, m, max_boxes))
    out, idx, obj_offs = ac.Guarded((cap, ld), "float32"), ac.Guarded((cap,), "int32"), ac.Guarded((m + 1,), "int32")
    good = list(_args(t, n, ld, B, m, max_boxes, cap, out.ptr, obj_offs.ptr, idx.ptr, ws.ptr, ws.ws_bytes))
    names = ["pts", "n", "ld", "offs", "batch", "boxes", "centre", "box_offs", "m", "max_boxes", "cap", "out", "obj_offs", "idx", "ws", "ws_bytes"]
    for kw in (dict(ld=2), dict(ld=0), dict(batch=0), dict(batch=-1), dict(n=-1), dict(m=-1), dict(max_boxes=-1), dict(cap=-1), dict(pts=None),
               dict(offs=None), dict(boxes=None), dict(centre=None), dict(box_offs=None), dict(out=None), dict(obj_offs=None), dict(ws=None),
               dict(ws_bytes=ws.ws_bytes - 1), dict(ws_bytes=8), dict(ws_bytes=0), dict(max_boxes=max_boxes + 1000)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert L().btc_cut_objects(*a, stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    for g in (out, idx, obj_offs):
        assert bool(g.poison_mask().all()) and g.guards_intact()
    assert ws.guards_intact() and bool((ws.tensor == 0xA5).all()), "a refused call touched the workspace"
