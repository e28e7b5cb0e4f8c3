"""The buffer contract of btc_count_in_boxes and btc_coverage_cells (include/btcdet_hip_infos.h), as the other contract files hold their
entry points to it: every output is a Guarded buffer (poisoned payload between two guard bands) with spare entries past its extent, the
workspace is garbage (both patterns), the call runs on a side stream.  Afterwards the stated extent is fully overwritten and equals the
numpy restatement, nothing past it and no guard is touched, the cells of a flagged job still hold the poison, the inputs hold the bits
they held, and the same call on the current stream with another dirty workspace gives the same bits.  Refused arguments return -1,
write nothing and enqueue nothing."""
import numpy as np
import pytest
import torch

import abi_contract as ac
import kitti_infos_ref as ir
import test_hip_kitti_infos as T

pytestmark = pytest.mark.gpu
SPARE = 5


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(a, b):
    return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------------ counts
def _count_inputs(sizes, nboxes, ld):
    pts, offs, blocks, boxes = T.make_batch(sizes, nboxes, ld=ld, seed=3)
    rows = [ir.hull_rows(b) for b in boxes if b.shape[0]]
    rows = np.concatenate(rows) if rows else np.zeros((0, 8), np.float32)
    box_offs = np.concatenate([[0], np.cumsum([b.shape[0] for b in boxes])]).astype(np.int32)
    t = {"pts": _dev(pts), "offs": _dev(offs.astype(np.int32)), "calib": _dev(blocks), "rows": _dev(rows), "box_offs": _dev(box_offs)}
    return t, (pts, offs, blocks, boxes)


def _count_args(t, n, ld, B, m, counts, fov, ws, ws_bytes):
    return (t["pts"].data_ptr() if n else None, n, ld, t["offs"].data_ptr(), B, t["calib"].data_ptr(), t["rows"].data_ptr() if m else None,
            t["box_offs"].data_ptr(), m, counts, fov, ws, ws_bytes)


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("ld", [4, 5])
@pytest.mark.parametrize("case", [((0,), (2,)), ((300, 0), (0, 0)), ((257, 0, 130), (3, 2, 0)), ((20,) * 9 + (400,), (1,) * 9 + (66,))],
                         ids=["n0", "m0", "387", "580"])
def test_count_in_boxes_buffer_contract(case, ld, garbage):
    from btcdet_amd._lib import check, stream_ptr
    sizes, nboxes = case
    t, (pts, offs, blocks, boxes) = _count_inputs(sizes, nboxes, ld)
    n, B, m = pts.shape[0], len(sizes), int(sum(nboxes))
    want, want_fov = ir.restate_counts(pts, offs, blocks, boxes)
    before = {k: v.clone() for k, v in t.items()}
    ws_bytes = L().btc_count_in_boxes_ws_bytes(n, B)
    ws = ac.Workspace(ws_bytes, garbage=garbage)
    counts, fov = ac.Guarded((m + SPARE,), "int32"), ac.Guarded((B + SPARE,), "int32")
    ac.call("btc_count_in_boxes", *_count_args(t, n, ld, B, m, counts.ptr, fov.ptr, ws.ptr, ws_bytes))
    print("rows", list(sizes), "boxes", list(nboxes), "ld", ld, "inside", int(want.sum()), "in view", want_fov.tolist())
    assert not bool(counts.poison_mask()[:m].any()) and bool(counts.poison_mask()[m:].all())
    assert not bool(fov.poison_mask()[:B].any()) and bool(fov.poison_mask()[B:].all())
    assert counts.tensor[:m].cpu().tolist() == want.tolist() and fov.tensor[:B].cpu().tolist() == want_fov.tolist()
    assert counts.guards_intact() and fov.guards_intact() and ws.guards_intact()
    for k, v in before.items():
        assert _same_bits(t[k], v), "input %s was written" % k
    # the same call on the current stream: ordinary buffers, another dirty workspace, no fov_rows
    c2 = torch.full((m + SPARE,), 7, dtype=torch.int32, device="cuda")
    w2 = torch.full((max(ws_bytes, 256),), 0x5A, dtype=torch.uint8, device="cuda")
    check(L().btc_count_in_boxes(*_count_args(t, n, ld, B, m, c2.data_ptr(), None, w2.data_ptr(), ws_bytes), stream_ptr()), "btc_count_in_boxes")
    torch.cuda.synchronize()
    assert torch.equal(c2[:m], counts.tensor[:m]) and bool((c2[m:] == 7).all())


def test_count_in_boxes_refusals_write_nothing():
    from btcdet_amd._lib import stream_ptr
    sizes, nboxes, ld = (257, 0, 130), (3, 2, 1), 4
    t, (pts, offs, blocks, boxes) = _count_inputs(sizes, nboxes, ld)
    n, B, m = pts.shape[0], len(sizes), int(sum(nboxes))
    ws = ac.Workspace(L().btc_count_in_boxes_ws_bytes(n, B))
    counts, fov = ac.Guarded((m,), "int32"), ac.Guarded((B,), "int32")
    good = list(_count_args(t, n, ld, B, m, counts.ptr, fov.ptr, ws.ptr, ws.ws_bytes))
    names = ["pts", "n", "ld", "offs", "batch", "calib", "boxes", "box_offs", "m", "counts", "fov", "ws", "ws_bytes"]
    for kw in (dict(ld=2), dict(ld=0), dict(batch=0), dict(batch=-1), dict(n=-1), dict(m=-1), dict(pts=None), dict(offs=None), dict(calib=None),
               dict(boxes=None), dict(box_offs=None), dict(counts=None), dict(ws=None), dict(ws_bytes=ws.ws_bytes - 1), dict(ws_bytes=8), dict(ws_bytes=0)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert L().btc_count_in_boxes(*a, stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    for g in (counts, fov):
        assert bool(g.poison_mask().all()) and g.guards_intact()
    assert ws.guards_intact() and bool((ws.tensor == 0xA5).all()), "a refused call touched the workspace"


# ------------------------------------------------------------------------------------------------------------------------- cells
def _cell_inputs(big, ld):
    """five jobs: an ordinary one, a template of no row, an object of no row, one past the key's range (flagged), one whose rows lie
    outside the banks (flagged); `big`: the first job has 4097 rows, so the call needs a table per job in the workspace"""
    rng = np.random.default_rng(41)
    n0 = 4097 if big else 130
    t0, o0, p0 = T.random_object(rng, n0, n0 - 7, (25.0, -6.0, -0.5), -1.1, extent=(30.0, 20.0, 6.0))
    t1, o1, p1 = T.random_object(rng, 60, 40, (330.0, 4.0, -1.0), 0.4)
    tmpl = np.concatenate([t0, t1])
    obj = np.zeros((o0.shape[0] + o1.shape[0], ld), np.float32)
    obj[:, 0:3] = np.concatenate([o0, o1])
    obj[:, 3:] = 0.25
    R = obj.shape[0]
    jobs = np.array([[0, n0, 0, n0 - 7], [0, 0, 0, 40], [0, 60, 0, 0], [n0, 60, n0 - 7, 40], [0, 60, R - 10, 40]], np.int32)
    pose = np.stack([p0, p0, p0, p1, p0])
    want, status = ir.restate_jobs(tmpl, obj, jobs[:4], pose[:4])
    return tmpl, obj, jobs, pose, want, status.tolist() + [2], n0


def _cell_args(t, T_, R, ld, J, max_rows, cells, status, ws, ws_bytes):
    return (t["tmpl"].data_ptr() if T_ else None, T_, t["obj"].data_ptr() if R else None, R, ld, t["jobs"].data_ptr() if J else None,
            t["pose"].data_ptr() if J else None, J, max_rows, cells, status, ws, ws_bytes)


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("ld", [4, 3])
@pytest.mark.parametrize("big", [False, True], ids=["lds", "workspace"])
def test_coverage_cells_buffer_contract(big, ld, garbage):
    from btcdet_amd._lib import check, stream_ptr
    tmpl, obj, jobs, pose, want, want_status, max_rows = _cell_inputs(big, ld)
    J = jobs.shape[0]
    t = {"tmpl": _dev(tmpl), "obj": _dev(obj), "jobs": _dev(jobs), "pose": _dev(pose)}
    before = {k: v.clone() for k, v in t.items()}
    ws_bytes = L().btc_coverage_cells_ws_bytes(J, max_rows)
    assert (ws_bytes > 256) == big
    ws = ac.Workspace(ws_bytes, garbage=garbage)
    cells, status = ac.Guarded((J + SPARE, 2), "int32"), ac.Guarded((J + SPARE,), "int32")
    ac.call("btc_coverage_cells", *_cell_args(t, tmpl.shape[0], obj.shape[0], ld, J, max_rows, cells.ptr, status.ptr, ws.ptr, ws_bytes))
    print("jobs", jobs.tolist(), "cells", cells.tensor[:J].cpu().tolist(), "status", status.tensor[:J].cpu().tolist())
    assert want_status == [0, 0, 0, 1, 2] and status.tensor[:J].cpu().tolist() == want_status and bool(status.poison_mask()[J:].all())
    assert cells.tensor[:3].cpu().tolist() == want[:3].tolist() and want[0, 0] > 50 and want[0, 1] > 50
    assert not bool(cells.poison_mask()[:3].any()) and bool(cells.poison_mask()[3:].all()), "a flagged job's cells are not written"
    assert cells.guards_intact() and status.guards_intact() and ws.guards_intact()
    for k, v in before.items():
        assert _same_bits(t[k], v), "input %s was written" % k
    c2 = torch.full((J, 2), 7, dtype=torch.int32, device="cuda")
    s2 = torch.full((J,), 7, dtype=torch.int32, device="cuda")
    w2 = torch.full((max(ws_bytes, 256),), 0x5A, dtype=torch.uint8, device="cuda")
    check(L().btc_coverage_cells(*_cell_args(t, tmpl.shape[0], obj.shape[0], ld, J, max_rows, c2.data_ptr(), s2.data_ptr(), w2.data_ptr(), ws_bytes),
                                 stream_ptr()), "btc_coverage_cells")
    torch.cuda.synchronize()
    assert torch.equal(s2, status.tensor[:J]) and torch.equal(c2[:3], cells.tensor[:3]) and bool((c2[3:] == 7).all())


def test_coverage_cells_refusals_write_nothing():
    from btcdet_amd._lib import stream_ptr
    tmpl, obj, jobs, pose, _, _, max_rows = _cell_inputs(True, 4)
    J = jobs.shape[0]
    t = {"tmpl": _dev(tmpl), "obj": _dev(obj), "jobs": _dev(jobs), "pose": _dev(pose)}
    ws = ac.Workspace(L().btc_coverage_cells_ws_bytes(J, max_rows))
    cells, status = ac.Guarded((J, 2), "int32"), ac.Guarded((J,), "int32")
    good = list(_cell_args(t, tmpl.shape[0], obj.shape[0], 4, J, max_rows, cells.ptr, status.ptr, ws.ptr, ws.ws_bytes))
    names = ["tmpl", "T", "obj", "R", "ld", "jobs", "pose", "J", "max_rows", "cells", "status", "ws", "ws_bytes"]
    for kw in (dict(J=-1), dict(T=-1), dict(R=-1), dict(ld=2), dict(ld=0), dict(max_rows=-1), dict(max_rows=2 ** 29), dict(ws=None), dict(jobs=None),
               dict(pose=None), dict(cells=None), dict(status=None), dict(tmpl=None), dict(obj=None), dict(ws_bytes=ws.ws_bytes - 1), dict(ws_bytes=256),
               dict(ws_bytes=0), dict(max_rows=2 * max_rows)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert L().btc_coverage_cells(*a, stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    for g in (cells, status):
        assert bool(g.poison_mask().all()) and g.guards_intact()
    assert ws.guards_intact() and bool((ws.tensor == 0xA5).all()), "a refused call touched the workspace"
    # J == 0 is legal and launches nothing
    assert L().btc_coverage_cells(None, 0, None, 0, 4, None, None, 0, 0, None, None, ws.ptr, ws.ws_bytes, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(cells.poison_mask().all()) and bool((ws.tensor == 0xA5).all())
