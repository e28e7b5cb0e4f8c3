"""The buffer contract of btc_nn_sqdist, btc_match_candidates and btc_select_templates (include/btcdet_hip_templates.h), as the other
contract files hold their entry points to it: every output is a Guarded buffer (poisoned payload between two guard bands) with spare
entries past the total, the workspace is garbage (both patterns), the call runs on a side stream.  Afterwards everything below the
totals is overwritten and equals the numpy restatement, everything past them and the guards are untouched, the inputs hold the bits
they held, and the same call on the current stream gives the same bits.  Refused arguments write nothing and enqueue nothing."""
import os

import numpy as np
import pytest
import torch

import abi_contract as ac
import template_ref as tr

pytestmark = pytest.mark.gpu
SPARE = 5
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "templates.npz")


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _class(name="Car", top_k=5, nbm=2):
    """the golden class as the arrays of the header: sets, seg, half, grid, own bitmaps, cand / iou (K = top_k + a trailing -1)"""
    gold = tr.load_golden(GOLD, name)
    sets = tr.golden_sets(gold, name)
    params = dict(tr.CLASS_PARAMS[name], max_num_bm=nbm)
    grid = tr.make_grid(sets)
    own = np.stack([tr.occ_words(s, grid) for s in sets])
    counts = np.array([tr.popcount(w) for w in own])
    cand, iou = tr.top_candidates(tr.box_iou_origin(gold["boxes"][:, 3:6]), counts > params["pnt_thresh"], top_k)
    cand, iou = np.concatenate([cand, cand[:, :1]], axis=1), np.concatenate([iou, iou[:, :1]], axis=1)
    cand[:, -1] = -1
    rows = np.array([s.shape[0] for s in sets], np.int64)
    seg = np.stack([np.cumsum(rows) - rows, rows], axis=1).astype(np.int32)
    half = np.stack([tr.half_dims(b) for b in gold["boxes"]])
    return dict(sets=sets, pts=np.concatenate(sets), seg=seg, half=half, grid=grid, own=own, cand=cand, iou=iou, params=params,
                obj=np.arange(len(sets), dtype=np.int32))


def _unchanged(t, before):
    for k, v in before.items():
        assert torch.equal(t[k].reshape(-1).view(torch.uint8), v.reshape(-1).view(torch.uint8)), "input %s was written" % k


def test_nn_sqdist_buffer_contract():
    from btcdet_amd._lib import check, stream_ptr
    c = _class()
    seg = c["seg"]
    pairs = np.array([[seg[a, 0], seg[a, 1], seg[b, 0], seg[b, 1]] for a, b in ((0, 1), (2, 2), (5, 3), (7, 0), (1, 9))], np.int32)
    offs = np.concatenate([[0], np.cumsum(pairs[:, 1])]).astype(np.int32)
    total, P, n = int(offs[-1]), pairs.shape[0], c["pts"].shape[0]
    want = np.concatenate([tr.nn_sqdist(c["sets"][a], c["sets"][b]) for a, b in ((0, 1), (2, 2), (5, 3), (7, 0), (1, 9))])
    t = {"pts": _t(c["pts"]), "pairs": _t(pairs), "offs": _t(offs)}
    before = {k: v.clone() for k, v in t.items()}
    out = ac.Guarded((total + SPARE,), "float32")
    args = (t["pts"].data_ptr(), n, t["pts"].data_ptr(), n, t["pairs"].data_ptr(), t["offs"].data_ptr(), P, total)
    ac.call("btc_nn_sqdist", *args, out.ptr)
    assert not bool(out.poison_mask()[:total].any()) and bool(out.poison_mask()[total:].all()) and out.guards_intact()
    assert out.tensor[:total].cpu().numpy().tobytes() == want.tobytes()
    _unchanged(t, before)
    o2 = torch.zeros((total + SPARE,), device="cuda")
    check(L().btc_nn_sqdist(*args, o2.data_ptr(), stream_ptr()), "btc_nn_sqdist")
    torch.cuda.synchronize()
    assert torch.equal(o2[:total].view(torch.int32), out.tensor[:total].view(torch.int32)) and not bool(o2[total:].any())


def _match_args(t, c, G, K):
    g, n, M = c["grid"], c["pts"].shape[0], c["seg"].shape[0]
    return (t["pts"].data_ptr(), n, t["seg"].data_ptr(), t["half"].data_ptr(), M, t["obj"].data_ptr(), t["cand"].data_ptr(), G, K, float(g["x0"]),
            float(g["y0"]), float(g["cell"]), g["nx"], g["ny"])


def test_match_candidates_buffer_contract():
    from btcdet_amd._lib import check, stream_ptr
    c = _class()
    G, K = c["cand"].shape
    W = tr.grid_words(c["grid"])
    want_md, want_so = tr.restate_match(c["sets"], list(c["half"]), c["obj"], c["cand"], c["grid"])
    t = {k: _t(c[k]) for k in ("pts", "seg", "half", "obj", "cand")}
    before = {k: v.clone() for k, v in t.items()}
    md, so = ac.Guarded((G * K + SPARE,), "float32"), ac.Guarded((G * K * W + SPARE,), "int32")
    ac.call("btc_match_candidates", *_match_args(t, c, G, K), md.ptr, so.ptr)
    assert not bool(md.poison_mask()[:G * K].any()) and bool(md.poison_mask()[G * K:].all()) and md.guards_intact()
    assert not bool(so.poison_mask()[:G * K * W].any()) and bool(so.poison_mask()[G * K * W:].all()) and so.guards_intact()
    assert md.tensor[:G * K].cpu().numpy().tobytes() == want_md.tobytes()
    assert so.tensor[:G * K * W].cpu().numpy().view(np.uint32).tobytes() == want_so.tobytes()
    _unchanged(t, before)
    m2, s2 = torch.zeros((G * K,), device="cuda"), torch.zeros((G * K * W,), dtype=torch.int32, device="cuda")
    check(L().btc_match_candidates(*_match_args(t, c, G, K), m2.data_ptr(), s2.data_ptr(), stream_ptr()), "btc_match_candidates")
    torch.cuda.synchronize()
    assert torch.equal(m2.view(torch.int32), md.tensor[:G * K].view(torch.int32)) and torch.equal(s2, so.tensor[:G * K * W])


def _select_setup(c):
    want_md, want_so = tr.restate_match(c["sets"], list(c["half"]), c["obj"], c["cand"], c["grid"])
    t = {k: _t(c[k]) for k in ("pts", "seg", "obj", "cand", "iou")}
    t["md"], t["so"], t["own"] = _t(want_md), _t(want_so.view(np.int32)), _t(c["own"].view(np.int32))
    p = c["params"]
    want = tr.restate_select(c["sets"], c["obj"], c["cand"], c["iou"], want_md, want_so, c["own"], p["max_num_bm"], 2000, 0.90, p["ex_coords_ratio"],
                             tr.nearest_sq(p["nearest_dist"]))
    return t, want


def _select_args(t, c, cap, out, src, offs, chosen, ws, ws_bytes):
    p, n, M = c["params"], c["pts"].shape[0], c["seg"].shape[0]
    G, K = c["cand"].shape
    return (t["pts"].data_ptr(), n, t["seg"].data_ptr(), M, t["obj"].data_ptr(), t["cand"].data_ptr(), t["iou"].data_ptr(), t["md"].data_ptr(),
            t["so"].data_ptr(), t["own"].data_ptr(), G, K, tr.grid_words(c["grid"]), p["max_num_bm"], 2000, 0.90, float(p["ex_coords_ratio"]),
            float(tr.nearest_sq(p["nearest_dist"])), int(c["seg"][:, 1].max()), cap, out, src, offs, chosen, ws, ws_bytes)


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("short", [False, True], ids=["spare", "short"])
def test_select_templates_buffer_contract(garbage, short):
    from btcdet_amd._lib import check, stream_ptr
    c = _class()
    t, (want_offs, want_chosen, want_out, want_src) = _select_setup(c)
    before = {k: v.clone() for k, v in t.items()}
    G, nbm = c["cand"].shape[0], c["params"]["max_num_bm"]
    total = int(want_offs[-1])
    cap = total - 11 if short else total + SPARE           # short: the capacity ends inside a template
    rows = total + SPARE
    written = min(cap, total)
    ws_bytes = L().btc_select_templates_ws_bytes(G, nbm, int(c["seg"][:, 1].max()))
    ws = ac.Workspace(ws_bytes, garbage=garbage)
    out, src = ac.Guarded((rows, 3), "float32"), ac.Guarded((rows, 2), "int32")
    offs, chosen = ac.Guarded((G + 1 + SPARE,), "int32"), ac.Guarded((G * nbm + SPARE,), "int32")
    ac.call("btc_select_templates", *_select_args(t, c, cap, out.ptr, src.ptr, offs.ptr, chosen.ptr, ws.ptr, ws_bytes))
    assert not bool(offs.poison_mask()[:G + 1].any()) and bool(offs.poison_mask()[G + 1:].all())
    assert not bool(chosen.poison_mask()[:G * nbm].any()) and bool(chosen.poison_mask()[G * nbm:].all())
    assert offs.tensor[:G + 1].cpu().tolist() == want_offs.tolist() and chosen.tensor[:G * nbm].cpu().tolist() == want_chosen.reshape(-1).tolist()
    assert not bool(out.poison_mask()[:written].any()) and bool(out.poison_mask()[written:].all()), "rows below the capacity, and only they"
    assert not bool(src.poison_mask()[:written].any()) and bool(src.poison_mask()[written:].all())
    assert out.tensor[:written].cpu().numpy().tobytes() == want_out[:written].tobytes()
    assert src.tensor[:written].cpu().numpy().tobytes() == want_src[:written].tobytes()
    assert out.guards_intact() and src.guards_intact() and offs.guards_intact() and chosen.guards_intact() and ws.guards_intact()
    _unchanged(t, before)
    o2, f2 = torch.zeros((rows, 3), device="cuda"), torch.zeros((G + 1,), dtype=torch.int32, device="cuda")
    c2 = torch.zeros((G * nbm,), dtype=torch.int32, device="cuda")
    w2 = torch.full((max(ws_bytes, 256),), 0x5A, dtype=torch.uint8, device="cuda")
    check(L().btc_select_templates(*_select_args(t, c, cap, o2.data_ptr(), None, f2.data_ptr(), c2.data_ptr(), w2.data_ptr(), ws_bytes), stream_ptr()),
          "btc_select_templates")
    torch.cuda.synchronize()
    assert torch.equal(f2, offs.tensor[:G + 1]) and torch.equal(c2, chosen.tensor[:G * nbm])
    assert torch.equal(o2[:written].view(torch.int32), out.tensor[:written].view(torch.int32)) and not bool(o2[written:].any())


def test_nothing_is_written_when_the_arguments_are_refused():
    from btcdet_amd._lib import stream_ptr
    c = _class()
    t, (want_offs, _, _, _) = _select_setup(c)
    t["half"] = _t(c["half"])
    G, K = c["cand"].shape
    nbm, W, total = c["params"]["max_num_bm"], tr.grid_words(c["grid"]), int(want_offs[-1])
    ws = ac.Workspace(L().btc_select_templates_ws_bytes(G, nbm, int(c["seg"][:, 1].max())))
    out, src = ac.Guarded((total, 3), "float32"), ac.Guarded((total, 2), "int32")
    offs, chosen = ac.Guarded((G + 1,), "int32"), ac.Guarded((G * nbm,), "int32")
    md, so, nn = ac.Guarded((G * K,), "float32"), ac.Guarded((G * K * W,), "int32"), ac.Guarded((total,), "float32")
    good = list(_select_args(t, c, total, out.ptr, src.ptr, offs.ptr, chosen.ptr, ws.ptr, ws.ws_bytes))
    names = ["pts", "n", "seg", "M", "obj", "cand", "iou", "md", "so", "own", "G", "K", "W", "nbm", "extra", "thr", "ratio", "nsq", "max_rows", "cap", "out",
             "src", "offs", "chosen", "ws", "ws_bytes"]
    for kw in (dict(G=-1), dict(M=-1), dict(n=-1), dict(cap=-1), dict(max_rows=-1), dict(extra=-1), dict(K=0), dict(K=8193), dict(W=0), dict(W=2049),
               dict(nbm=0), dict(nbm=9), dict(pts=None), dict(seg=None), dict(obj=None), dict(cand=None), dict(iou=None), dict(md=None), dict(so=None),
               dict(own=None), dict(out=None), dict(offs=None), dict(chosen=None), dict(ws=None), dict(ws_bytes=ws.ws_bytes - 1), dict(ws_bytes=0),
               dict(max_rows=1 << 20)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert L().btc_select_templates(*a, stream_ptr()) == -1, kw
    good = list(_match_args(t, c, G, K)) + [md.ptr, so.ptr]
    names = ["pts", "n", "seg", "half", "M", "obj", "cand", "G", "K", "x0", "y0", "cell", "nx", "ny", "md", "so"]
    for kw in (dict(n=-1), dict(M=-1), dict(G=-1), dict(K=0), dict(nx=0), dict(ny=0), dict(cell=0.0), dict(nx=4096, ny=4096), dict(pts=None), dict(seg=None),
               dict(half=None), dict(obj=None), dict(cand=None), dict(md=None), dict(so=None)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert L().btc_match_candidates(*a, stream_ptr()) == -1, kw
    n = c["pts"].shape[0]
    pairs, po = _t(np.array([[0, total, 0, n]], np.int32)), _t(np.array([0, total], np.int32))
    good = [t["pts"].data_ptr(), n, t["pts"].data_ptr(), n, pairs.data_ptr(), po.data_ptr(), 1, total, nn.ptr]
    names = ["q", "nq", "t", "nt", "pairs", "offs", "P", "out_rows", "out"]
    for kw in (dict(P=-1), dict(nq=-1), dict(nt=-1), dict(out_rows=-1), dict(q=None), dict(t=None), dict(pairs=None), dict(offs=None), dict(out=None)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert L().btc_nn_sqdist(*a, stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    for g in (out, src, offs, chosen, md, so, nn):
        assert bool(g.poison_mask().all()) and g.guards_intact()
    assert ws.guards_intact() and bool((ws.tensor == 0xA5).all()), "a refused call touched the workspace"
