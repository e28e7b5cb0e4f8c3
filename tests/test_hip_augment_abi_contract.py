"""The buffer contract of btc_augment_batch and btc_world_transform (include/btcdet_hip_augment.h), as the other contract files hold
their entry points to it: out, out_pre and out_offsets are Guarded buffers (poisoned payload between two guard bands), the workspace is
garbage (both patterns), the call runs on a side stream.  Afterwards rows [0, n') are fully overwritten and equal the host functions'
result, rows past n' and the guards are untouched, the inputs hold the bits they held, and the same call on the current stream gives the
same bits.  Refused arguments write nothing."""
import numpy as np
import pytest
import torch

import abi_contract as ac
import test_hip_augment as T

pytestmark = pytest.mark.gpu
LD = 4
SPARE = 5          # rows of capacity beyond n_rows + pasted rows: there is always a row past n'


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _case(n_rows, R, n_obj):
    from btcdet_amd.device_augmentor import removal_rows
    rng = np.random.default_rng(100 * n_rows + 10 * R + n_obj)
    sizes = [n_rows - n_rows // 2, n_rows // 2]
    scans = [T._scene(rng, s, LD) for s in sizes]
    boxes = [T._boxes(rng, R) if R else np.zeros((0, 7), np.float32), T._boxes(rng, R // 2) if R // 2 else np.zeros((0, 7), np.float32)]
    bank = T._bank(rng, LD)
    objects = [[(3, 7, (10.25, -3.5, -0.75), 0.125), (11, 1, (30.0, 5.0, -1.0), 0.0)], [(20, 20, (33.0, -7.0, -0.5), 0.25)]] if n_obj else [[], []]
    d0, h0 = T._ops()
    d1, h1 = T._ops(order="rs", flip=False)
    flat = [o for per in objects for o in per]
    host = {"pts": np.concatenate(scans).reshape(-1, LD), "offs": np.cumsum([0] + sizes).astype(np.int32),
            "rm": np.concatenate([removal_rows(b) for b in boxes]).reshape(-1, 8).astype(np.float32),
            "rm_offs": np.cumsum([0] + [len(b) for b in boxes]).astype(np.int32), "bank": bank,
            "first": np.array([o[0] for o in flat] + [0], np.int32), "rows": np.array([o[1] for o in flat] + [0], np.int32),
            "shift": np.array([list(o[2]) + [o[3]] for o in flat] + [[0.0] * 4], np.float64),
            "obj_offs": np.cumsum([0] + [len(per) for per in objects]).astype(np.int32),
            "ops": np.array([list(o) + [0.0] * (4 - len(o)) for per in (d0, d1) for o in per], np.float32),
            "op_offs": np.array([0, len(d0), len(d0) + len(d1)], np.int32)}
    want = [T.host_expect(scans[b], boxes[b], objects[b], bank, (h0, h1)[b]) for b in range(2)]
    paste = int(sum(o[1] for o in flat))
    return host, want, len(flat), paste


def _args(t, n_rows, n_obj, paste, cap, out, pre, offs, ws, ws_bytes):
    from btcdet_amd._lib import ptr
    return (ptr(t["pts"]), n_rows, LD, ptr(t["offs"]), 2, ptr(t["rm"]), ptr(t["rm_offs"]), ptr(t["bank"]), t["bank"].shape[0], ptr(t["first"]),
            ptr(t["rows"]), ptr(t["shift"]), ptr(t["obj_offs"]), n_obj, paste, ptr(t["ops"]), ptr(t["op_offs"]), cap, out, pre, offs, ws, ws_bytes)


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("n_rows,R,n_obj", [(n, r, o) for n in (1, 257) for r in (0, 65) for o in (0, 3)])
def test_augment_batch_buffer_contract(n_rows, R, n_obj, garbage):
    from btcdet_amd._lib import check, ptr, stream_ptr
    host, want, n_flat, paste = _case(n_rows, R, n_obj)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    before = {k: v.clone() for k, v in t.items()}
    cap = n_rows + paste + SPARE
    ws_bytes = L().btc_augment_ws_bytes(n_rows, 2, n_flat)
    ws = ac.Workspace(ws_bytes, garbage=garbage)
    out, pre, offs = ac.Guarded((cap, LD), "float32"), ac.Guarded((cap, LD), "float32"), ac.Guarded((3,), "int32")
    s = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    rc = L().btc_augment_batch(*_args(t, n_rows, n_flat, paste, cap, out.ptr, pre.ptr, offs.ptr, ws.ptr, ws_bytes), s.cuda_stream)
    s.synchronize()
    assert rc == 0, "rc %d: %s" % (rc, L().btc_last_error().decode("utf-8", "replace"))
    assert not bool(offs.poison_mask().any())
    bounds = offs.tensor.cpu().numpy()
    total = sum(w[0].shape[0] for w in want)
    print("n_rows", n_rows, "R", R, "objects", n_flat, "kept", [w[2] for w in want], "offsets", bounds.tolist())
    assert bounds.tolist() == [0, want[0][0].shape[0], total]
    for g, idx, what in ((out, 0, "out"), (pre, 1, "out_pre")):
        assert not bool(g.poison_mask()[:total].any()), "%s: a row below n' was left unwritten" % what
        assert bool(g.poison_mask()[total:].all()), "%s: a row past n' was written" % what
        got = g.tensor.cpu().numpy()
        for b in range(2):
            T._same(got[bounds[b]:bounds[b + 1]], want[b][idx], (what, b))
    assert out.guards_intact() and pre.guards_intact() and offs.guards_intact() and ws.guards_intact()
    for k, v in before.items():
        assert torch.equal(t[k].reshape(-1).view(torch.uint8), v.reshape(-1).view(torch.uint8)), "input %s was written" % k
    # the same call on the current stream (ordinary buffers, no guards) gives the same bits
    o2, p2 = torch.zeros((cap, LD), device="cuda"), torch.zeros((cap, LD), device="cuda")
    f2 = torch.zeros((3,), dtype=torch.int32, device="cuda")
    w2 = torch.empty((max(ws_bytes, 256),), dtype=torch.uint8, device="cuda")
    check(L().btc_augment_batch(*_args(t, n_rows, n_flat, paste, cap, ptr(o2), ptr(p2), ptr(f2), ptr(w2), ws_bytes), stream_ptr()), "btc_augment_batch")
    torch.cuda.synchronize()
    assert torch.equal(f2, offs.tensor)
    assert torch.equal(o2[:total].view(torch.int32), out.tensor[:total].view(torch.int32))
    assert torch.equal(p2[:total].view(torch.int32), pre.tensor[:total].view(torch.int32))


@pytest.mark.parametrize("n_rows", [1, 44, 257])
def test_world_transform_buffer_contract(n_rows):
    from btcdet_amd import data_side
    rng = np.random.default_rng(n_rows)
    sizes = [n_rows - n_rows // 3, n_rows // 3]
    sets = [rng.uniform(-30, 30, (s, 3)).astype(np.float32) for s in sizes]
    c, s_ = T._cos_sin(0.45)
    ops = np.array([[2, np.float32(0.96875), 0, 0], [3, c, s_, 1.0 if sizes[0] < 45 else 0.0], [1, 0, 0, 0], [3, c, s_, 1.0 if sizes[1] < 45 else 0.0]],
                   np.float32)
    t = {"in": torch.from_numpy(np.concatenate(sets)).cuda(), "offs": torch.tensor([0, sizes[0], n_rows], dtype=torch.int32, device="cuda"),
         "ops": torch.from_numpy(ops).cuda(), "op_offs": torch.tensor([0, 2, 4], dtype=torch.int32, device="cuda")}
    before = {k: v.clone() for k, v in t.items()}
    out = ac.Guarded((n_rows, 3), "float32")
    ac.call("btc_world_transform", t["in"].data_ptr(), n_rows, 3, t["offs"].data_ptr(), 2, t["ops"].data_ptr(), t["op_offs"].data_ptr(), out.ptr)
    assert not bool(out.poison_mask().any()) and out.guards_intact()
    a = sets[0].copy()
    a[:, :3] *= 0.96875
    a = data_side.rotate_points_along_z(a[np.newaxis], np.array([0.45]))[0]
    b = sets[1].copy()
    b[:, 1] = -b[:, 1]
    b = data_side.rotate_points_along_z(b[np.newaxis], np.array([0.45]))[0]
    T._same(out.tensor.cpu().numpy(), np.concatenate([a, b]), "world_transform")
    for k, v in before.items():
        assert torch.equal(t[k], v), "input %s was written" % k


def test_nothing_is_written_when_the_arguments_are_refused():
    from btcdet_amd._lib import stream_ptr
    n_rows, R, n_obj = 257, 65, 3
    host, want, n_flat, paste = _case(n_rows, R, n_obj)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    cap = n_rows + paste + SPARE
    ws = ac.Workspace(L().btc_augment_ws_bytes(n_rows, 2, n_flat))
    out, pre, offs = ac.Guarded((cap, LD), "float32"), ac.Guarded((cap, LD), "float32"), ac.Guarded((3,), "int32")
    good = list(_args(t, n_rows, n_flat, paste, cap, out.ptr, pre.ptr, offs.ptr, ws.ptr, ws.ws_bytes))
    names = ["pts", "n_rows", "ld", "offs", "batch", "rm", "rm_offs", "bank", "bank_rows", "first", "rows", "shift", "obj_offs", "n_obj", "paste", "ops",
             "op_offs", "cap", "out", "pre", "out_offs", "ws", "ws_bytes"]
    for kw in (dict(ld=2), dict(batch=0), dict(n_rows=-1), dict(n_obj=-1), dict(paste=-1), dict(bank_rows=-1), dict(cap=n_rows + paste - 1),
               dict(paste=2 ** 31, cap=2 ** 32), dict(pts=None), dict(offs=None), dict(rm_offs=None), dict(bank=None), dict(first=None), dict(rows=None),
               dict(shift=None), dict(obj_offs=None), dict(op_offs=None), dict(out=None), dict(out_offs=None), dict(ws=None),
               dict(ws_bytes=ws.ws_bytes - 1), dict(ws_bytes=8)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert L().btc_augment_batch(*a, stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    for g in (out, pre, offs):
        assert bool(g.poison_mask().all()) and g.guards_intact()
    assert ws.guards_intact() and bool((ws.tensor == 0xA5).all())
