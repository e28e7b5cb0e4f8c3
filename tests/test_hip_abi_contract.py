"""The C ABI's buffer contract, entry point by entry point (include/btcdet_hip.h): every output is a poisoned buffer between guard
bands (tests/abi_contract.py), every workspace holds garbage beyond its documented zero head, every call runs through ctypes on a
non-default stream.  Each case compares every element of every output with a reference that shares no code with the kernel (the
oracle, numpy, torch in float64; the tolerance of the entry point's existing test where it is not bit-exact), checks that slots the
header says are not written still hold the poison, that no guard was touched and that persistent workspace heads are zero again --
then calls again with the SAME workspace and a smaller geometry.

test_poisoned_allocations_leave_the_training_step_bit_identical covers the wrappers' own allocations: the same training step with
torch.empty / empty_like / new_empty returning poisoned memory must give the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import abi_contract as ac
from oracle import oracle as orc
from test_hip_core import rand_indices

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
c_f32p, c_i32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)


def L():
    from btcdet_amd._lib import lib
    return lib()


def T(a):
    """a device copy of a numpy array, kept alive until the case ends (an inline temporary would go back to the caching allocator
    before the call, and the next input could take its block)"""
    return keep(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))


def B16(a):
    return keep(T(a).bfloat16())


def keep(t):
    _KEEP.append(t)
    return t


def G(shape, dtype):
    g = ac.Guarded(shape, dtype, DEV)
    _LIVE.append(g)
    return g


def W(nbytes, garbage, zero_head=0):
    w = ac.Workspace(nbytes, zero_head=zero_head, garbage=garbage, device=DEV)
    _LIVE.append(w)
    return w


def H(g):
    return g.tensor.cpu().numpy() if g.dtype != torch.bfloat16 else g.tensor.float().cpu().numpy()


def fp(a):
    return np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(c_f32p)


def i3p(v):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), (3,))).ctypes.data_as(c_i32p)


def still_poison(g, sl=slice(None)):
    assert bool(g.poison_mask()[sl].all()), "a slot the header leaves untouched was written"


_LIVE, _KEEP = [], []


class tuned(object):
    def __init__(self, **kv):
        self.kv = {int(k[1:]): v for k, v in kv.items()}

    def __enter__(self):
        for k, v in self.kv.items():
            assert L().btc_tune_set(k, v) == 0

    def __exit__(self, *a):
        for k in self.kv:
            L().btc_tune_set(k, 0)


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["gA5", "gFF"])
@pytest.mark.parametrize("case", sorted(ac.CASES))
def test_contract(case, garbage):
    del _LIVE[:], _KEEP[:]
    try:
        globals()["case_" + case](garbage)
        torch.cuda.synchronize()
        bad = [i for i, g in enumerate(_LIVE) if not g.guards_intact()]
    finally:
        torch.cuda.synchronize()
        del _LIVE[:], _KEEP[:]
    assert not bad, "guard bands overwritten (buffers %s of this case)" % bad


# ============================================================================================================ voxelization, prestep
def case_voxelize(garbage):
    rngr, vs, maxp, maxv = [0, 0, 0, 10, 10, 10], [1.0, 0.5, 2.0], 7, 150
    grid = np.round((np.array(rngr[3:]) - rngr[:3]) / np.array(vs)).astype(np.int32)
    rng = np.random.default_rng(1)
    big = [rng.uniform(-0.5, 10.5, (n, 5)).astype(np.float32) for n in (4001, 1, 0, 2015)]
    small = [rng.uniform(-0.5, 10.5, (n, 5)).astype(np.float32) for n in (63, 17)]
    ws = W(L().btc_voxelize_ws_bytes(sum(len(s) for s in big), len(big), maxp), garbage)
    og = orc.VoxelGeneratorV2(vs, rngr, maxp, maxv)
    for scenes in (big, small):
        pts = np.concatenate(scenes)
        offs = np.cumsum([0] + [len(s) for s in scenes]).astype(np.int32)
        B, cap = len(scenes), len(scenes) * maxv
        v, c, nm, tot = G((cap, maxp, 5), "float32"), G((cap, 4), "int32"), G((cap,), "int32"), G((1,), "int32")
        ac.call("btc_voxelize", T(pts).data_ptr(), len(pts), 5, 0, 0, 5, T(offs).data_ptr(), B, fp(rngr), fp(vs), i3p(grid), maxp, maxv,
                v.ptr, c.ptr, nm.ptr, tot.ptr, ws.ptr, ws.ws_bytes)
        row = 0
        for b, p in enumerate(scenes):
            r = og.generate(p)
            m = r["voxel_num"]
            np.testing.assert_array_equal(H(c)[row:row + m, 0], b)
            np.testing.assert_array_equal(H(c)[row:row + m, 1:], r["coordinates"])
            np.testing.assert_array_equal(H(nm)[row:row + m], r["num_points_per_voxel"])
            np.testing.assert_array_equal(H(v)[row:row + m], r["voxels"])
            row += m
        assert int(H(tot)[0]) == row
        for g in (v, c, nm):
            still_poison(g, slice(row, None))      # rows >= M are left untouched


def case_range_mask_gather(garbage):
    rng = np.random.default_rng(2)
    lim = np.array([0.0, -20.0, 40.0, 20.0], np.float32)
    big, small = [rng.uniform(-10, 50, (n, 4)).astype(np.float32) for n in (1601, 0, 65)], [rng.uniform(-10, 50, (n, 4)).astype(np.float32) for n in (15,)]
    ws = W(L().btc_range_mask_ws_bytes(sum(len(s) for s in big)), garbage)
    for scenes in (big, small):
        pts = np.concatenate(scenes)
        pre = (pts[:, :3] * 2 + 1).astype(np.float32)
        n, B = len(pts), len(scenes)
        offs = np.cumsum([0] + [len(s) for s in scenes]).astype(np.int32)
        out, outb, noffs, keep = G((n, 4), "float32"), G((n, 3), "float32"), G((B + 1,), "int32"), G((n,), "int32")
        ac.call("btc_range_mask_compact", T(pts).data_ptr(), T(pre).data_ptr(), n, 4, 3, T(offs).data_ptr(), B, fp(lim), out.ptr, outb.ptr,
                noffs.ptr, keep.ptr, ws.ptr, ws.ws_bytes)
        keep_ref, new = [], [0]
        for b in range(B):
            p = pts[offs[b]:offs[b + 1]]
            m = (p[:, 0] >= lim[0]) & (p[:, 0] <= lim[2]) & (p[:, 1] >= lim[1]) & (p[:, 1] <= lim[3])
            keep_ref.append(offs[b] + np.nonzero(m)[0])
            new.append(new[-1] + int(m.sum()))
        kr = np.concatenate(keep_ref).astype(np.int32)
        k = len(kr)
        np.testing.assert_array_equal(H(noffs), new)
        np.testing.assert_array_equal(H(keep)[:k], kr)
        np.testing.assert_array_equal(H(out)[:k], pts[kr])
        np.testing.assert_array_equal(H(outb)[:k], pre[kr])
        for g in (out, outb, keep):
            still_poison(g, slice(k, None))
        # gather_rows: a permutation with two bad indices (zero rows, counted)
        idx = rng.permutation(n).astype(np.int32)
        if n >= 2:
            idx[0], idx[-1] = -3, n + 5
        gout, bad = G((n, 4), "float32"), G((1,), "int32")
        bad.tensor.zero_()
        ac.call("btc_gather_rows", T(pts).data_ptr(), T(idx).data_ptr(), n, 4, n, gout.ptr, bad.ptr)
        ok = (idx >= 0) & (idx < n)
        ref = np.zeros((n, 4), np.float32)
        ref[ok] = pts[idx[ok]]
        np.testing.assert_array_equal(H(gout), ref)
        assert int(H(bad)[0]) == int((~ok).sum())


def case_cart_to_occ_coords(garbage):
    rng = np.random.default_rng(3)
    for n in (4097, 1, 0):
        p = rng.uniform(-40, 40, (n, 5)).astype(np.float32)
        for mode, fn in ((1, orc.absxyz_2_cylinxyz_np), (2, orc.absxyz_2_spherexyz_np)):
            out = G((n, 5), "float32")
            ac.call("btc_cart_to_occ_coords", T(p).data_ptr(), out.ptr, n, 5, mode)
            np.testing.assert_allclose(H(out), fn(p), rtol=2e-6, atol=2e-5)
            np.testing.assert_array_equal(H(out)[:, 3:], p[:, 3:])


def case_voxel_shift_col(garbage):
    rng = np.random.default_rng(4)
    for m, B in ((1025, 3), (1, 1)):
        vox = rng.standard_normal((m, 5, 4)).astype(np.float32)
        coords = np.zeros((m, 4), np.int32)
        coords[:, 0] = np.sort(rng.integers(0, B, m))
        rot = rng.standard_normal(B).astype(np.float32)
        g = G((m + 3, 5, 4), "float32")          # three rows past m must stay poison
        g.tensor[:m].copy_(T(vox))
        ac.call("btc_voxel_shift_col", g.ptr, T(coords).data_ptr(), m, 5, 4, 1, T(rot).data_ptr(), -1.0)
        ref = vox.copy()
        ref[:, :, 1] = vox[:, :, 1] - rot[coords[:, 0]][:, None]
        np.testing.assert_array_equal(H(g)[:m], ref)
        still_poison(g, slice(m, None))


# ============================================================================================================ geometry
def case_rulebook_subm(garbage):
    rng = np.random.default_rng(5)
    shape = (7, 12, 11)
    n_big = 1601
    ws = W(L().btc_rulebook_subm_ws_bytes(n_big), garbage)
    for n, B, k, d in ((n_big, 3, (3, 3, 3), (1, 1, 1)), (63, 2, (1, 3, 3), (1, 1, 1)), (17, 1, (3, 3, 3), (1, 2, 2)), (1, 1, (3, 3, 3), (1, 1, 1))):
        idx = rand_indices(rng, n, B, shape)
        K = int(np.prod(k))
        no, ni = G((n, K), "int32"), G((n, K), "int32")
        ac.call("btc_rulebook_subm", T(idx).data_ptr(), n, B, i3p(shape), i3p(k), i3p(d), no.ptr, ni.ptr, ws.ptr, ws.ws_bytes)
        _, o_out, o_in, _ = orc.rulebook(idx, shape, k, 1, 0, d, orc.MODE_SUBM)
        np.testing.assert_array_equal(H(no), o_out)
        np.testing.assert_array_equal(H(ni), o_in)
    # nbr_in NULL: nbr_out alone
    no = G((n, K), "int32")
    ac.call("btc_rulebook_subm", T(idx).data_ptr(), n, B, i3p(shape), i3p(k), i3p(d), no.ptr, None, ws.ptr, ws.ws_bytes)
    np.testing.assert_array_equal(H(no), o_out)


def _rb_conv(idx, B, shape, k, s, p, d, mode, ws):
    osh = orc.out_shape(shape, k, s, p, d, mode).astype(np.int32)
    n = len(idx)
    K = int(np.prod(np.broadcast_to(k, (3,))))
    cnt = G((1,), "int32")
    t = T(idx.reshape(-1, 4))
    args = (t.data_ptr(), n, B, i3p(shape), i3p(osh), i3p(k), i3p(s), i3p(p), i3p(d), mode)
    ac.call("btc_rulebook_conv_count", *args, cnt.ptr, ws.ptr, ws.ws_bytes)
    n_out = int(H(cnt)[0])
    oi, no, ni = G((n_out, 4), "int32"), G((n_out, K), "int32"), G((n, K), "int32")
    ac.call("btc_rulebook_conv_fill", *args, n_out, oi.ptr, no.ptr, ni.ptr, ws.ptr, ws.ws_bytes)
    o_idx, o_out, o_in, o_sh = orc.rulebook(idx.reshape(-1, 4), shape, k, s, p, d, mode)
    assert n_out == len(o_idx)
    np.testing.assert_array_equal(H(oi), o_idx)
    np.testing.assert_array_equal(H(no), o_out)
    np.testing.assert_array_equal(H(ni), o_in)


def case_rulebook_conv(garbage):
    rng = np.random.default_rng(6)
    CONV, TR = orc.MODE_CONV, orc.MODE_TRANSPOSE
    geoms = [((9, 15, 13), 3, (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), CONV, 1601),    # big first: the workspace is sized by it
             ((3, 8, 7), 2, (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), TR, 65),
             ((5, 10, 8), 1, (3, 1, 1), (2, 1, 1), (0, 0, 0), (1, 1, 1), CONV, 47),             # the pooling geometry of the heads
             ((4, 6, 8), 2, (2, 2, 2), (2, 2, 2), (0, 0, 0), (1, 1, 1), CONV, 1),
             ((4, 6, 8), 1, (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), CONV, 0)]
    wsb = max(L().btc_rulebook_conv_ws_bytes(B, i3p(orc.out_shape(sh, k, s, p, d, m))) for sh, B, k, s, p, d, m, _ in geoms)
    ws = W(wsb, garbage)
    for sh, B, k, s, p, d, m, n in geoms:
        _rb_conv(rand_indices(rng, n, B, sh), B, sh, k, s, p, d, m, ws)


def _chain_layers(shape, spec):
    from btcdet_amd._lib import BtcChainLayer
    arr = (BtcChainLayer * len(spec))()
    cur = list(shape)
    geo = []
    for i, (kind, mode, k, s, p) in enumerate(spec):
        l = arr[i]
        l.kind, l.ref, l.mode = kind, -1, mode
        osh = list(orc.out_shape(cur, k, s, p, 1, mode)) if kind == 1 else cur
        l.in_shape[:], l.out_shape[:] = cur, osh
        l.k[:], l.s[:], l.p[:], l.d[:] = [k] * 3, [s] * 3 if kind == 1 else [1] * 3, [p] * 3 if kind == 1 else [0] * 3, [1] * 3
        geo.append((list(cur), k, s, p, mode))
        cur = osh
    return arr, geo


def case_chain(garbage):
    SUBM, CONV, TR = orc.MODE_SUBM, orc.MODE_CONV, orc.MODE_TRANSPOSE
    spec = [(1, CONV, 3, 2, 1), (0, SUBM, 3, 1, 0), (1, CONV, 3, 2, 1), (0, SUBM, 3, 1, 0), (1, TR, 3, 2, 1)]
    shape = (17, 40, 60)
    rng = np.random.default_rng(7)
    big, small = (rand_indices(rng, 6001, 2, shape), 2), (rand_indices(rng, 63, 3, shape), 3)
    layers, geo = _chain_layers(shape, spec)
    n = len(spec)
    wsb = max(L().btc_chain_ws_bytes(layers, n, B, len(idx)) for idx, B in (big, small))
    ws = W(wsb, garbage)
    for idx, B in (big, small):
        rng.shuffle(idx)                      # arbitrary input order (the chain's input level is hashed)
        cap = (ctypes.c_int64 * n)()
        assert L().btc_chain_caps(layers, n, B, len(idx), cap) == 0
        outs = [G((cap[i], 4), "int32") if spec[i][0] == 1 else None for i in range(n)]
        cnt = G((n,), "int32")
        p_out = (ctypes.POINTER(ctypes.c_int32) * n)(*[ctypes.cast(o.ptr, c_i32p) if o else None for o in outs])
        t = T(idx)
        ac.call("btc_chain_levels", t.data_ptr(), len(idx), B, layers, n, p_out, cap, cnt.ptr, ws.ptr, ws.ws_bytes)
        hc = H(cnt)
        counts = (ctypes.c_int32 * n)(*[int(hc[i]) if spec[i][0] == 1 else 0 for i in range(n)])
        cur, maps = idx, []
        for i, (kind, mode, k, s, p) in enumerate(spec):
            o_idx, o_out, o_in, _ = orc.rulebook(cur, geo[i][0], k, s, p, 1, mode)
            if kind == 1:
                assert int(hc[i]) == len(o_idx)
                np.testing.assert_array_equal(H(outs[i])[:len(o_idx)], o_idx)
                still_poison(outs[i], slice(len(o_idx), None))
            maps.append((o_idx, o_out, o_in, len(cur)))
            cur = o_idx if kind == 1 else cur
        nbo = [G((len(m[0]) if spec[i][0] == 1 else m[3], 27), "int32") for i, m in enumerate(maps)]
        nbi = [G((m[3], 27), "int32") if spec[i][0] == 1 else None for i, m in enumerate(maps)]
        fo = [G((len(m[0]),), "int32") if spec[i][0] == 1 else None for i, m in enumerate(maps)]
        fi = [G((m[3],), "int32") if spec[i][0] == 1 else None for i, m in enumerate(maps)]
        pp = lambda lst: (ctypes.POINTER(ctypes.c_int32) * n)(*[ctypes.cast(o.ptr, c_i32p) if o else None for o in lst])
        ac.call("btc_chain_maps", t.data_ptr(), len(idx), B, layers, n, counts, p_out, pp(nbo), pp(nbi), pp(fo), pp(fi), ws.ptr, ws.ws_bytes)
        for i, (o_idx, o_out, o_in, _) in enumerate(maps):
            np.testing.assert_array_equal(H(nbo[i]), o_out, err_msg="layer %d nbr_out" % i)
            if nbi[i] is not None:
                np.testing.assert_array_equal(H(nbi[i]), o_in, err_msg="layer %d nbr_in" % i)
                for f, mp in ((fo[i], o_out), (fi[i], o_in)):
                    first = np.where((mp >= 0).any(1), np.argmax(mp >= 0, axis=1), 27)
                    np.testing.assert_array_equal(np.minimum(H(f), 27), first, err_msg="layer %d first keys" % i)


def case_pairs_from_nbr(garbage):
    rng = np.random.default_rng(8)
    shape = (9, 15, 13)
    res = []
    for n, B in ((1601, 3), (17, 1)):
        idx = rand_indices(rng, n, B, shape)
        o_idx, o_out, _, _ = orc.rulebook(idx, shape, 3, 2, 1, 1, orc.MODE_CONV)
        res.append((n, o_out))
    ws = W(max(L().btc_pairs_from_nbr_ws_bytes(len(o), 27) for _, o in res), garbage)
    for n_in, o_out in res:
        pairs, num = G((2, 27, n_in), "int32"), G((27,), "int32")
        ac.call("btc_pairs_from_nbr", T(o_out).data_ptr(), len(o_out), 27, n_in, pairs.ptr, num.ptr, ws.ptr, ws.ws_bytes)
        cp, cn = orc.canonical_pairs(o_out)
        np.testing.assert_array_equal(H(num), cn)
        P = H(pairs)
        for kk in range(27):
            np.testing.assert_array_equal(P[:, kk, :cn[kk]], cp[kk])
            assert np.all(P[:, kk, cn[kk]:] == -1)


def _first_keys(m, K):
    return np.where((m >= 0).any(1), np.argmax(m >= 0, axis=1), K)


def _check_order(order, maps, K):
    off = 0
    for m in maps:
        n = len(m)
        o = order[off:off + n]
        assert np.array_equal(np.sort(o), np.arange(n)), "not a permutation"
        key = _first_keys(m, K)
        for b0 in range(0, n, 2048):                     # stable counting sort inside blocks of 2048 rows
            blk = np.arange(b0, min(n, b0 + 2048))
            np.testing.assert_array_equal(o[b0:b0 + len(blk)], blk[np.argsort(key[blk], kind="stable")])
        off += n


def case_row_orders(garbage):
    rng = np.random.default_rng(9)
    shape = (9, 30, 28)
    maps = []
    for n, B in ((5001, 2), (65, 1), (1, 1)):
        idx = rand_indices(rng, n, B, shape)
        _, o_out, o_in, _ = orc.rulebook(idx, shape, 3, 2, 1, 1, orc.MODE_CONV)
        maps += [o_out, o_in]
    for sub in (maps, maps[2:]):
        ts = [T(m) for m in sub]
        n_tot = sum(len(m) for m in sub)
        nbrs = (ctypes.c_void_p * len(sub))(*[t.data_ptr() for t in ts])
        ns = np.array([len(m) for m in sub], np.int32)
        ks = np.full(len(sub), 27, np.int32)
        order = G((n_tot + 5,), "int32")
        ac.call("btc_row_orders", nbrs, ns.ctypes.data_as(c_i32p), ks.ctypes.data_as(c_i32p), len(sub), order.ptr)
        _check_order(H(order)[:n_tot], sub, 27)
        still_poison(order, slice(n_tot, None))
        keys = [T(_first_keys(m, 27).astype(np.int32)) for m in sub]
        firsts = (ctypes.c_void_p * len(sub))(*[k.data_ptr() if j % 2 == 0 else None for j, k in enumerate(keys)])
        order2 = G((n_tot,), "int32")
        ac.call("btc_row_orders_keyed", nbrs, firsts, ns.ctypes.data_as(c_i32p), ks.ctypes.data_as(c_i32p), len(sub), order2.ptr)
        np.testing.assert_array_equal(H(order2), H(order)[:n_tot])


# ============================================================================================================ conv
def _conv_problem(rng, n, B, kind, cin, cout, shape=(8, 20, 18)):
    idx = rand_indices(rng, n, B, shape)
    s = 1 if kind == "subm" else 2
    mode = orc.MODE_SUBM if kind == "subm" else orc.MODE_CONV
    o_idx, o_out, o_in, _ = orc.rulebook(idx, shape, 3, s, 1, 1, mode)
    feat = rng.standard_normal((len(idx), cin)).astype(np.float32)
    Wt = (rng.standard_normal((27, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    dout = rng.standard_normal((len(o_idx), cout)).astype(np.float32)
    return feat, Wt, dout, o_out, o_in


def case_conv_fwd_dgrad(garbage):
    rng = np.random.default_rng(10)
    with tuned(k14=1):
        for n, kind, cin, cout in ((1601, "subm", 16, 32), (2049, "subm", 4, 16), (63, "conv", 32, 16), (17, "subm", 32, 3), (1, "subm", 16, 16)):
            feat, Wt, dout, o_out, o_in = _conv_problem(rng, n, 2 if n > 1 else 1, kind, cin, cout)
            bias = rng.standard_normal(cout).astype(np.float32)
            no, ni = len(o_out), len(o_in)
            out, din = G((no, cout), "float32"), G((ni, cin), "float32")
            ac.call("btc_conv_fwd", T(feat).data_ptr(), T(Wt).data_ptr(), T(bias).data_ptr(), T(o_out).data_ptr(), no, 27, cin, cout, out.ptr)
            np.testing.assert_array_equal(H(out), orc.conv_fwd(feat, Wt.reshape(3, 3, 3, cin, cout), bias, o_out))
            ac.call("btc_conv_dgrad", T(dout).data_ptr(), T(Wt).data_ptr(), T(o_in).data_ptr(), ni, 27, cin, cout, din.ptr)
            np.testing.assert_array_equal(H(din), orc.conv_dgrad(dout, Wt.reshape(3, 3, 3, cin, cout), o_in))
            if cin % 16 == 0 and cout % 16 == 0:      # bf16 activations: bf16 of the same fmaf chain over the bf16 inputs
                fb, db = orc.bf16_round(feat), orc.bf16_round(dout)
                outb, dinb = G((no, cout), "bfloat16"), G((ni, cin), "bfloat16")
                ac.call("btc_conv_fwd_bf16", B16(fb).data_ptr(), T(Wt).data_ptr(), T(bias).data_ptr(), T(o_out).data_ptr(), no, 27,
                        cin, cout, outb.ptr)
                np.testing.assert_array_equal(H(outb), orc.bf16_round(orc.conv_fwd(fb, Wt.reshape(3, 3, 3, cin, cout), bias, o_out)))
                ac.call("btc_conv_dgrad_bf16", B16(db).data_ptr(), T(Wt).data_ptr(), T(o_in).data_ptr(), ni, 27, cin, cout, dinb.ptr)
                np.testing.assert_array_equal(H(dinb), orc.bf16_round(orc.conv_dgrad(db, Wt.reshape(3, 3, 3, cin, cout), o_in)))


def _bf16_weights(Wt, multi=False):
    K, cin, cout = Wt.shape
    w, wt = G((K, cin, cout), "bfloat16"), G((K, cout, cin), "bfloat16")
    tw = T(Wt)
    if not multi:
        ac.call("btc_weights_to_bf16", tw.data_ptr(), K, cin, cout, w.ptr, wt.ptr)
    else:
        one = lambda v: (ctypes.c_void_p * 1)(v)
        ac.call("btc_weights_to_bf16_multi", one(tw.data_ptr()), one(w.ptr), one(wt.ptr), np.array([K], np.int32).ctypes.data_as(c_i32p),
                np.array([cin], np.int32).ctypes.data_as(c_i32p), np.array([cout], np.int32).ctypes.data_as(c_i32p), 1)
    r = orc.bf16_round(Wt)
    np.testing.assert_array_equal(H(w), r)
    np.testing.assert_array_equal(H(wt), r.transpose(0, 2, 1))
    return w, wt


def _bound_bf16w(got, src, Wb, nbr, transpose, bias=None):
    """|got - float64 product of the bf16 operands| <= bf16 rounding of the result + 2e-6 of the scale (test_hip_bf16_mfma.py)"""
    K = Wb.shape[0]
    n = nbr.shape[0]
    ref = np.zeros((n, Wb.shape[1] if transpose else Wb.shape[2]), np.float64)
    if bias is not None:
        ref += bias.astype(np.float64)
    for k in range(K):
        r = np.nonzero(nbr[:, k] >= 0)[0]
        w = Wb[k].astype(np.float64)
        ref[r] += src[nbr[r, k]].astype(np.float64) @ (w.T if transpose else w)
    scale = np.abs(ref).max() + 1e-12
    assert np.all(np.abs(got - ref) <= np.abs(ref) * 2.0 ** -8 + 2e-6 * scale)


def case_conv_bf16w(garbage):
    rng = np.random.default_rng(11)
    for n, multi in ((1601, False), (17, True)):
        feat, Wt, dout, o_out, o_in = _conv_problem(rng, n, 2, "subm", 32, 32)
        w, wt = _bf16_weights(Wt, multi)
        fb, db = orc.bf16_round(feat), orc.bf16_round(dout)
        out, din = G((len(o_out), 32), "bfloat16"), G((len(o_in), 32), "bfloat16")
        ac.call("btc_conv_fwd_bf16w", B16(fb).data_ptr(), wt.ptr, None, T(o_out).data_ptr(), len(o_out), 27, 32, 32, out.ptr)
        _bound_bf16w(H(out), fb, orc.bf16_round(Wt), o_out, False)
        ac.call("btc_conv_dgrad_bf16w", B16(db).data_ptr(), w.ptr, T(o_in).data_ptr(), len(o_in), 27, 32, 32, din.ptr)
        _bound_bf16w(H(din), db, orc.bf16_round(Wt), o_in, True)


def _split_weights(Wt, multi):
    K, cin, cout = Wt.shape
    ws_, wt_ = G((3, K, cin, cout), "bfloat16"), G((3, K, cout, cin), "bfloat16")
    tw = T(Wt)
    if not multi:
        ac.call("btc_weights_split3", tw.data_ptr(), K, cin, cout, ws_.ptr, wt_.ptr)
    else:
        one = lambda v: (ctypes.c_void_p * 1)(v)
        ac.call("btc_weights_split3_multi", one(tw.data_ptr()), one(ws_.ptr), one(wt_.ptr), np.array([K], np.int32).ctypes.data_as(c_i32p),
                np.array([cin], np.int32).ctypes.data_as(c_i32p), np.array([cout], np.int32).ctypes.data_as(c_i32p), 1)
    s = H(ws_).astype(np.float64)
    np.testing.assert_array_equal(s[0] + s[1] + s[2], Wt.astype(np.float64))     # an exact split
    np.testing.assert_array_equal(H(wt_), H(ws_).transpose(0, 1, 3, 2))
    return ws_, wt_


def case_conv_apply(garbage):
    """btc_conv_apply_ordered / _src in every operand mode and pass, with a row-order hint; row counts on both sides of the
    split-operand policy threshold (btc_conv_split_wanted) and of conv_apply_ws's 2048 rows"""
    rng = np.random.default_rng(12)
    thr = next(n for n in range(16, 200000, 16) if L().btc_conv_split_wanted(27, 32, 32, n) == 1) if \
        L().btc_conv_split_wanted(27, 32, 32, 199984) == 1 else None
    sizes = [1601, 2047, 2049, 17]
    if thr is not None and thr < 30000:
        sizes += [thr - 1, thr + 15]
    for n in sizes:
        feat, Wt, dout, o_out, o_in = _conv_problem(rng, n, 2, "subm", 32, 32, shape=(12, 48, 44))
        bias = rng.standard_normal(32).astype(np.float32)
        nr = len(o_out)
        order = rng.permutation(nr).astype(np.int32)
        to, tf, tW, tb = T(o_out), T(feat), T(Wt), T(bias)
        Wr = Wt.reshape(3, 3, 3, 32, 32)
        ref_f, ref_d = orc.conv_fwd(feat, Wr, bias, o_out), orc.conv_dgrad(dout, Wr, o_in)
        for pass_, src, ref, b in ((0, tf, ref_f, tb), (1, T(dout), ref_d, None), (2, T(dout), ref_d, None)):
            nbr = to if pass_ != 1 else T(o_in)
            out = G((nr, 32), "float32")
            ac.call("btc_conv_apply_ordered", pass_, 0, src.data_ptr(), tW.data_ptr(), b.data_ptr() if b is not None else None,
                    nbr.data_ptr(), T(order).data_ptr(), nr, 27, 32, 32, out.ptr)
            np.testing.assert_array_equal(H(out), ref)
            # bf16 activations, fp32 weights: bit-exact over the bf16 inputs
            sb = orc.bf16_round(src.cpu().numpy())
            outb = G((nr, 32), "bfloat16")
            ac.call("btc_conv_apply_src", pass_, 1, B16(sb).data_ptr(), nr, tW.data_ptr(), b.data_ptr() if b is not None else None,
                    nbr.data_ptr(), None, nr, 27, 32, 32, outb.ptr)
            f = orc.conv_fwd if pass_ == 0 else orc.conv_dgrad
            refb = f(sb, Wr, bias, o_out) if pass_ == 0 else f(sb, Wr, o_in)
            np.testing.assert_array_equal(H(outb), orc.bf16_round(refb))
            # bf16 operands
            w, wt = _bf16_weights(Wt)
            outq = G((nr, 32), "bfloat16")
            ac.call("btc_conv_apply_ordered", pass_, 2, B16(sb).data_ptr(), (wt if pass_ == 0 else w).ptr,
                    b.data_ptr() if b is not None else None, nbr.data_ptr(), T(order).data_ptr(), nr, 27, 32, 32, outq.ptr)
            _bound_bf16w(H(outq), sb, orc.bf16_round(Wt), o_out if pass_ == 0 else (o_in if pass_ == 1 else o_out[:, ::-1]), pass_ != 0,
                         bias if pass_ == 0 else None)
            # split fp32 operands: within 2e-6 of the result's scale of the exact chain (test_hip_split.py)
            wsp, wtp = _split_weights(Wt, multi=(pass_ == 2))
            outs = G((nr, 32), "float32")
            ac.call("btc_conv_apply_src", pass_, 3, src.data_ptr(), src.shape[0], (wtp if pass_ == 0 else wsp).ptr,
                    b.data_ptr() if b is not None else None, nbr.data_ptr(), T(order).data_ptr(), nr, 27, 32, 32, outs.ptr)
            assert np.abs(H(outs) - ref).max() <= 2e-6 * (np.abs(ref).max() + 1e-12)


def _bn_ref(x64, gamma, beta, rm, rv, relu, momentum=0.01, eps=1e-3):
    mean = x64.mean(0)
    var = x64.var(0, unbiased=False)
    y = (x64 - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    if relu:
        y = torch.relu(y)
    n = x64.shape[0]
    rm2 = (1 - momentum) * rm.double() + momentum * mean
    rv2 = (1 - momentum) * rv.double() + momentum * x64.var(0, unbiased=True) if n > 1 else rv.double()
    return y, mean, torch.rsqrt(var + eps), rm2, rv2


def case_conv_bn_relu(garbage):
    rng = np.random.default_rng(13)
    fuse = W(L().btc_bn_fuse_ws_bytes(), garbage, zero_head=L().btc_bn_fuse_ws_bytes())
    bnw = W(L().btc_bn_ws_bytes(32), garbage, zero_head=256)
    with tuned(k14=1):
        for n, src_form in ((2049, False), (1601, True), (63, False), (1, True)):
            feat, Wt, dout, o_out, o_in = _conv_problem(rng, n, 2 if n > 1 else 1, "subm", 16, 32)
            nr = len(o_out)
            gamma, beta = T(rng.uniform(0.5, 1.5, 32).astype(np.float32)), T(rng.uniform(-0.5, 0.5, 32).astype(np.float32))
            rm, rv = T(rng.uniform(-0.1, 0.1, 32).astype(np.float32)), T(rng.uniform(0.5, 1.5, 32).astype(np.float32))
            rm0, rv0 = rm.clone(), rv.clone()
            nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
            x, y, sm, sr = G((nr, 32), "float32"), G((nr, 32), "float32"), G((32,), "float32"), G((32,), "float32")
            args = (T(feat).data_ptr(),) + ((len(feat),) if src_form else ()) + (T(Wt).data_ptr(), None, T(o_out).data_ptr(), None, nr, 27, 16, 32,
                                                                                x.ptr, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                                                                nbt.data_ptr(), 0.01, 1e-3, 1, y.ptr, sm.ptr, sr.ptr, bnw.ptr, bnw.ws_bytes, fuse.ptr)
            ac.call("btc_conv_bn_relu_fwd_src" if src_form else "btc_conv_bn_relu_fwd", 0, *args)
            xr = orc.conv_fwd(feat, Wt.reshape(3, 3, 3, 16, 32), None, o_out)
            np.testing.assert_array_equal(H(x), xr)
            yr, mr, rr, rm2, rv2 = _bn_ref(T(xr).double(), gamma, beta, rm0, rv0, True)
            tol = dict(rtol=2e-5, atol=2e-5)
            np.testing.assert_allclose(H(y), yr.cpu().numpy(), **tol)
            np.testing.assert_allclose(H(sm), mr.cpu().numpy(), **tol)
            np.testing.assert_allclose(H(sr), rr.cpu().numpy(), rtol=2e-5)
            np.testing.assert_allclose(rm.cpu().numpy(), rm2.cpu().numpy(), **tol)
            if nr > 1:
                np.testing.assert_allclose(rv.cpu().numpy(), rv2.cpu().numpy(), **tol)
            assert int(nbt.item()) == 1
            assert fuse.head_zero() and bnw.head_zero(), "persistent workspace head not left zero"


def case_conv_wgrad(garbage):
    """every wgrad form against a float64 product: <= 1e-4 of the scale (tests/test_hip_core.py); the slab form and its multi-job
    reduction equal the one-call form bit for bit (tests/test_hip_wgrad_x.py)"""
    rng = np.random.default_rng(14)
    probs = [(1601, 32, 32, "subm"), (4097, 32, 16, "subm"), (2049, 32, 5, "subm"), (2100, 6, 16, "conv"), (63, 16, 32, "conv"), (1, 16, 16, "subm")]
    wsb = 0
    built = []
    for n, cin, cout, kind in probs:
        feat, Wt, dout, o_out, o_in = _conv_problem(rng, n, 2 if n > 1 else 1, kind, cin, cout, shape=(12, 48, 44))
        built.append((feat, dout, o_out, o_in, cin, cout))
        wsb = max(wsb, L().btc_conv_wgrad_ws_bytes(len(o_out), 27, cin, cout, len(feat)))
    ws = W(wsb, garbage)
    for feat, dout, o_out, o_in, cin, cout in built:
        ref = np.zeros((27, cin, cout))
        for k in range(27):
            r = np.nonzero(o_out[:, k] >= 0)[0]
            ref[k] = feat[o_out[r, k]].astype(np.float64).T @ dout[r].astype(np.float64)
        scale = np.abs(ref).max() + 1e-6
        tf, td, to, ti = T(feat), T(dout), T(o_out), T(o_in)
        nr, ns = len(o_out), len(feat)
        dw = G((27, cin, cout), "float32")
        ac.call("btc_conv_wgrad", tf.data_ptr(), td.data_ptr(), to.data_ptr(), nr, ti.data_ptr(), ns, 27, cin, cout, dw.ptr, ws.ptr, wsb)
        assert np.abs(H(dw) - ref).max() <= 1e-4 * scale
        dwo = G((27, cin, cout), "float32")
        oo, oi = T(rng.permutation(nr).astype(np.int32)), T(rng.permutation(ns).astype(np.int32))
        ac.call("btc_conv_wgrad_ordered", 0, tf.data_ptr(), td.data_ptr(), to.data_ptr(), nr, ti.data_ptr(), ns, oo.data_ptr(), oi.data_ptr(),
                27, cin, cout, dwo.ptr, ws.ptr, wsb)
        assert np.abs(H(dwo) - ref).max() <= 1e-4 * scale
        # two-call form: slabs in ws, then the reduction
        dws = G((27, cin, cout), "float32")
        nsl = ctypes.c_int(-1)
        ac.call("btc_conv_wgrad_slabs", 0, tf.data_ptr(), td.data_ptr(), to.data_ptr(), nr, ti.data_ptr(), ns, None, None, 27, cin, cout,
                dws.ptr, ws.ptr, wsb, ctypes.byref(nsl))
        if nsl.value > 0:
            still_poison(dws)                    # dW untouched until the reduction
            ac.call("btc_wgrad_reduce_multi", (ctypes.c_void_p * 1)(ws.ptr), (ctypes.c_void_p * 1)(dws.ptr), (ctypes.c_int * 1)(nsl.value),
                    (ctypes.c_longlong * 1)(27 * cin * cout), 1)
        assert torch.equal(dws.tensor, dw.tensor), "slabs + reduce != one call"
        if cin % 16 == 0 and cout % 16 == 0:
            fb, db = orc.bf16_round(feat), orc.bf16_round(dout)
            refb = np.zeros((27, cin, cout))
            for k in range(27):
                r = np.nonzero(o_out[:, k] >= 0)[0]
                refb[k] = fb[o_out[r, k]].astype(np.float64).T @ db[r].astype(np.float64)
            dwb = G((27, cin, cout), "float32")
            ac.call("btc_conv_wgrad_bf16", B16(fb).data_ptr(), B16(db).data_ptr(), to.data_ptr(), nr, ti.data_ptr(), ns,
                    27, cin, cout, dwb.ptr, ws.ptr, wsb)
            assert np.abs(H(dwb) - refb).max() <= 1e-4 * (np.abs(refb).max() + 1e-6)


def case_maxpool(garbage):
    rng = np.random.default_rng(15)
    shape = (9, 14, 12)
    for n, B, C in ((1601, 2, 16), (63, 1, 2), (1, 1, 3)):
        idx = rand_indices(rng, n, B, shape)
        _, o_out, o_in, _ = orc.rulebook(idx, shape, 3, 2, 1, 1, orc.MODE_CONV)
        feat = (rng.random((n, C)) - 0.2).astype(np.float32)
        feat[rng.random(feat.shape) < 0.3] = 0.5
        out, din = G((len(o_out), C), "float32"), G((n, C), "float32")
        ac.call("btc_maxpool_fwd", T(feat).data_ptr(), T(o_out).data_ptr(), len(o_out), 27, C, out.ptr)
        ref = orc.maxpool_fwd(feat, o_out)
        np.testing.assert_array_equal(H(out), ref)
        dout = rng.standard_normal(ref.shape).astype(np.float32)
        ac.call("btc_maxpool_bwd", T(feat).data_ptr(), T(ref).data_ptr(), T(dout).data_ptr(), T(o_in).data_ptr(), n, 27, C, din.ptr)
        np.testing.assert_allclose(H(din), orc.maxpool_bwd(feat, ref, dout, o_in), rtol=1e-6, atol=1e-6)


def case_dense(garbage):
    rng = np.random.default_rng(16)
    shape = (5, 14, 12)
    for n, B, ca, cb in ((1601, 2, 2, 3), (1, 1, 1, 1)):
        idx = rand_indices(rng, n, B, shape)
        feat = rng.standard_normal((n, ca + cb)).astype(np.float32)
        ti = T(idx)
        d = G((B, ca + cb) + shape, "float32")
        d.tensor.zero_()                        # the caller zero-fills (header)
        ac.call("btc_dense_fwd", T(feat).data_ptr(), ti.data_ptr(), n, ca + cb, i3p(shape), d.ptr)
        np.testing.assert_array_equal(H(d), orc.dense(feat, idx, B, shape))
        g = rng.standard_normal((B, ca + cb) + shape).astype(np.float32)
        df = G((n, ca + cb), "float32")
        ac.call("btc_dense_bwd", T(g).data_ptr(), ti.data_ptr(), n, ca + cb, i3p(shape), df.ptr)
        cell = g[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]]
        np.testing.assert_array_equal(H(df), cell)
        da, db = G((B, ca) + shape, "float32"), G((B, cb) + shape, "float32")
        da.tensor.zero_()
        db.tensor.zero_()
        ac.call("btc_dense_split_fwd", T(feat).data_ptr(), ti.data_ptr(), n, ca, cb, i3p(shape), da.ptr, db.ptr)
        np.testing.assert_array_equal(H(da), orc.dense(feat[:, :ca], idx, B, shape))
        np.testing.assert_array_equal(H(db), orc.dense(feat[:, ca:], idx, B, shape))
        for ga, gb in ((g[:, :ca], g[:, ca:]), (g[:, :ca], None)):
            dfs = G((n, ca + cb), "float32")
            ac.call("btc_dense_split_bwd", T(ga).data_ptr(), T(gb).data_ptr() if gb is not None else None, ti.data_ptr(), n, ca, cb, i3p(shape),
                    dfs.ptr)
            exp = cell.copy()
            if gb is None:
                exp[:, ca:] = 0
            np.testing.assert_array_equal(H(dfs), exp)


def case_cat_pad(garbage):
    rng = np.random.default_rng(17)
    for dt, esz in (("float32", 4), ("bfloat16", 2)):
        for n, ca, cb, cout in ((1601, 32, 2, 48), (17, 17, 3, 32), (1, 32, 2, 34), (0, 32, 2, 48)):
            a, b = torch.randn(n, ca).to(DEV).to(getattr(torch, dt)), torch.randn(n, cb).to(DEV).to(getattr(torch, dt))
            out = G((n, cout), dt)
            ac.call("btc_cat_pad_fwd", a.data_ptr(), ca, b.data_ptr(), cb, n, cout, esz, out.ptr)
            ref = torch.nn.functional.pad(torch.cat((a, b), 1), (0, cout - ca - cb))
            assert torch.equal(out.tensor, ref)
            g = torch.randn(n, cout).to(DEV).to(getattr(torch, dt))
            da, db = G((n, ca), dt), G((n, cb), dt)
            ac.call("btc_cat_pad_bwd", g.data_ptr(), cout, n, esz, da.ptr, ca, db.ptr, cb)
            assert torch.equal(da.tensor, g[:, :ca]) and torch.equal(db.tensor, g[:, ca:ca + cb])


# ============================================================================================================ normalisation, reductions
def case_bn_relu(garbage):
    rng = np.random.default_rng(18)
    ws = W(L().btc_bn_ws_bytes(64), garbage, zero_head=256)
    for n, c, relu, training, bf in ((70001, 64, True, True, False), (2049, 34, False, True, True), (17, 16, True, False, False), (1, 32, True, False, True)):
        x = T((rng.standard_normal((n, c)) * 2 + 0.5).astype(np.float32))
        dy = T(rng.standard_normal((n, c)).astype(np.float32))
        if bf:
            x, dy = x.bfloat16(), dy.bfloat16()
        gamma, beta = T(rng.uniform(0.5, 1.5, c).astype(np.float32)), T(rng.uniform(-0.5, 0.5, c).astype(np.float32))
        rm, rv = T(rng.uniform(-0.1, 0.1, c).astype(np.float32)), T(rng.uniform(0.5, 1.5, c).astype(np.float32))
        rm0, rv0 = rm.clone(), rv.clone()
        nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
        dt = "bfloat16" if bf else "float32"
        y, sm, sr = G((n, c), dt), G((c,), "float32"), G((c,), "float32")
        ac.call("btc_bn_relu_fwd_bf16" if bf else "btc_bn_relu_fwd", x.data_ptr(), n, c, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
                rv.data_ptr(), nbt.data_ptr(), 0.01, 1e-3, int(training), int(relu), y.ptr, sm.ptr, sr.ptr, ws.ptr, ws.ws_bytes)
        x64 = x.double()
        if training:
            yr, mr, rr, rm2, rv2 = _bn_ref(x64, gamma, beta, rm0, rv0, relu)
        else:
            mr, rr = rm0.double(), torch.rsqrt(rv0.double() + 1e-3)
            yr = (x64 - mr) * rr * gamma.double() + beta.double()
            yr = torch.relu(yr) if relu else yr
            rm2, rv2 = rm0.double(), rv0.double()
        tol = dict(rtol=2e-5, atol=2e-5) if not bf else dict(rtol=2 ** -7, atol=2e-5)
        np.testing.assert_allclose(H(y), yr.cpu().numpy(), **tol)
        stol = dict(rtol=2e-5, atol=2e-5) if not bf else dict(rtol=1e-5, atol=1e-6)     # (tests/test_hip_core.py, tests/test_hip_bf16.py)
        np.testing.assert_allclose(rm.cpu().numpy(), rm2.cpu().numpy(), **stol)
        np.testing.assert_allclose(rv.cpu().numpy(), rv2.cpu().numpy(), **stol)
        assert int(nbt.item()) == int(training)
        if training:
            np.testing.assert_allclose(H(sm), mr.cpu().numpy(), rtol=2e-5, atol=2e-5)
            np.testing.assert_allclose(H(sr), rr.cpu().numpy(), rtol=2e-5)
        assert ws.head_zero()
        # backward against float64 autograd of the same formula
        dx, dg, dbt = G((n, c), dt), G((c,), "float32"), G((c,), "float32")
        ac.call("btc_bn_relu_bwd_bf16" if bf else "btc_bn_relu_bwd", x.data_ptr(), y.ptr, dy.data_ptr(), n, c, gamma.data_ptr(),
                sm.ptr, sr.ptr, int(training), int(relu), dx.ptr, dg.ptr, dbt.ptr, ws.ptr, ws.ws_bytes)
        xa = x64.clone().requires_grad_(True)
        ga, ba = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        if training:
            mean, var = xa.mean(0), xa.var(0, unbiased=False)
            ya = (xa - mean) / torch.sqrt(var + 1e-3) * ga + ba
        else:
            ya = (xa - rm0.double()) * torch.rsqrt(rv0.double() + 1e-3) * ga + ba
        mask = (y.tensor.float() > 0).double() if relu else 1.0     # ReLU's gradient as the kernel sees it: through its own y
        (ya * mask * dy.double()).sum().backward()
        np.testing.assert_allclose(H(dx), xa.grad.cpu().numpy(), **(dict(rtol=2e-4, atol=2e-5) if not bf else dict(rtol=2 ** -7, atol=1e-3)))
        np.testing.assert_allclose(H(dg), ga.grad.cpu().numpy(), rtol=2e-4, atol=2e-3)
        np.testing.assert_allclose(H(dbt), ba.grad.cpu().numpy(), rtol=2e-4, atol=2e-3)
        assert ws.head_zero()


def case_col_sum(garbage):
    ws = W(L().btc_bn_ws_bytes(128), garbage, zero_head=256)
    g = torch.Generator(device="cpu").manual_seed(19)
    for n, c, bf in ((150001, 32, False), (2049, 128, True), (1, 3, False), (17, 16, True)):
        x = (torch.randn((n, c), generator=g) * 3 + 1).to(DEV)
        if bf:
            x = x.bfloat16()
        out = G((c,), "float32")
        ac.call("btc_col_sum_bf16" if bf else "btc_col_sum", x.data_ptr(), n, c, out.ptr, ws.ptr, ws.ws_bytes)
        np.testing.assert_allclose(H(out), x.double().sum(0).cpu().numpy(), rtol=2e-6, atol=2e-3)
        assert ws.head_zero()


def case_sumsq2(garbage):
    ws = W(L().btc_sumsq2_ws_bytes(), garbage, zero_head=256)
    g = torch.Generator(device="cpu").manual_seed(20)
    for na, nb, bbf in ((2 * 64 * 50 * 44, 7001, True), (17, 0, False), (1, 1, False)):
        a = torch.randn(na, generator=g).to(DEV)
        b = torch.randn(max(nb, 1), generator=g).to(DEV)[:nb]
        b = b.bfloat16() if bbf else b
        out = G((1,), "float32")
        ka, kb = 1e-3 / na, 2e-3 / max(nb, 1)
        ac.call("btc_sumsq2_fwd", a.data_ptr(), na, 0, ka, b.data_ptr() if nb else None, nb, int(bbf), kb, out.ptr, ws.ptr, ws.ws_bytes)
        ref = ka * a.double().pow(2).sum() + kb * b.double().pow(2).sum()
        assert abs(float(H(out)[0]) - float(ref)) <= 2e-6 * abs(float(ref))
        assert ws.head_zero()
        gr = torch.tensor([3.0], device=DEV)
        da, db = G((na,), "float32"), G((nb,), "bfloat16" if bbf else "float32")
        ac.call("btc_sumsq2_bwd", a.data_ptr(), na, 0, 2 * ka, da.ptr, b.data_ptr() if nb else None, nb, int(bbf), 2 * kb,
                db.ptr if nb else None, gr.data_ptr())
        fa = torch.tensor(3.0 * 2 * ka, device=DEV, dtype=torch.float32)
        assert torch.allclose(da.tensor, a * fa, rtol=1e-6, atol=0)
        if nb:
            fb = torch.tensor(3.0 * 2 * kb, device=DEV, dtype=torch.float32).to(b.dtype)
            assert torch.allclose(db.tensor.float(), (b * fb).float(), rtol=1e-2 if bbf else 1e-6, atol=0)


# ============================================================================================================ occupancy
def case_occ_targets(garbage):
    """the wrapper allocates the outputs; here every torch.empty it makes is poisoned ("need not be initialised", header) and the result
    must still equal the reference-pinned oracle exactly where tests/test_hip_occupancy.py is exact; the device back-projection table
    (btc_occ_backproject_lut, into a guarded buffer) equals the one the wrapper builds"""
    from golden_batch import golden_batch
    from oracle import occ_oracle
    from btcdet_amd.config import load_cfg
    from test_hip_occupancy import EXACT_MASKS, run_gpu
    cfg = load_cfg()
    bd = golden_batch()[2]
    ref = occ_oracle.OccOracle(cfg).targets(bd)
    with poisoned_allocations() as count:
        out, _ = run_gpu(bd, cfg, torch.device(DEV), backproject="torch")
        torch.cuda.synchronize()
    assert count[0] > 0
    for k in EXACT_MASKS + ["general_cls_loss_mask_float", "general_reg_loss_mask_float"]:
        assert torch.equal(out[k].cpu().to(ref[k].dtype), ref[k]), k
    for k in ["pos_mask", "occ_fore_cls_mask", "occ_mirr_cls_mask", "occ_bm_cls_mask", "general_reg_loss_mask", "forebox_label",
              "fore_voxelwise_mask", "bm_voxelwise_mask"]:
        assert torch.equal(out[k].cpu() > 0, ref[k] > 0), k
    assert int(out["pos_all_num"]) == int(ref["pos_all_num"])
    assert float((out["res_mtrx"].cpu() - ref["res_mtrx"]).abs().max()) <= 1e-3
    # the table
    from btcdet_amd.occ_targets import OccTargets3D, cylinder_voxel_centers
    import copy
    c2 = copy.deepcopy(cfg)
    c2.MODEL.OCC.TARGETS["BACKPROJECT"] = "device"
    d = c2.DATA_CONFIG
    occ_range = np.array(d.OCC.POINT_CLOUD_RANGE, dtype=np.float32)
    grid = np.round((occ_range[3:6] - occ_range[0:3]) / np.array(d.OCC.VOXEL_SIZE)).astype(np.int64)
    mod = OccTargets3D(model_cfg=c2.MODEL.OCC, voxel_size=d.OCC.VOXEL_SIZE, point_cloud_range=occ_range, data_cfg=d, grid_size=grid,
                       num_class=1, voxel_centers=cylinder_voxel_centers(grid, occ_range, d.OCC.VOXEL_SIZE, torch.device(DEV))).to(DEV)
    table = mod.backproject_table(torch.device(DEV))
    sg = list(mod._cfg.sphere_grid)
    lut = G((sg[2], sg[1], sg[0]), "int32")
    ac.call("btc_occ_backproject_lut", ctypes.byref(mod._cfg), lut.ptr)
    assert torch.equal(lut.tensor.view(-1), table.view(-1))


def case_occ_prob(garbage):
    rng = np.random.default_rng(21)
    for B, ncell in ((2, 9 * 157 * 209), (1, 17), (3, 1)):
        logit = rng.standard_normal((B, 2, ncell)).astype(np.float32) * 3
        mask = (rng.random((B, ncell)) < 0.5).astype(np.uint8)
        prob = G((B, ncell), "float32")
        ac.call("btc_occ_prob", T(logit).data_ptr(), T(mask).data_ptr(), B, ncell, prob.ptr)
        l64 = logit.astype(np.float64)
        ref = 1.0 / (1.0 + np.exp(l64[:, 0] - l64[:, 1])) * mask
        np.testing.assert_allclose(H(prob), ref, rtol=1e-6, atol=1e-7)


def _occ_loss_ref(logit, res, tgt, pos, cm, cw, rm, rw, beta, w_cls, w_res):
    l = torch.from_numpy(logit).double().requires_grad_(True)
    r = torch.from_numpy(res).double().requires_grad_(True)
    p = torch.softmax(l, dim=1) + 1e-6
    onehot = torch.stack([1.0 - torch.from_numpy(pos).double(), torch.from_numpy(pos).double()], 1)
    fl = (onehot * (-(1 - p) ** 2 * torch.log(p))).sum(1)
    cwm = torch.from_numpy(cw).double() * torch.from_numpy(cm).double()
    cls = w_cls * (fl * cwm).sum() / torch.clamp(cwm.sum(), min=1.0)
    n = (r - torch.from_numpy(tgt).double()).abs()
    sl1 = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta).sum(1)
    rwm = torch.from_numpy(rw).double() * torch.from_numpy(rm).double()
    reg = w_res * (sl1 * rwm).sum() / torch.clamp(rwm.sum(), min=1.0)
    return l, r, cls, reg


def case_occ_loss(garbage):
    rng = np.random.default_rng(22)
    ws = W(L().btc_occ_loss_ws_bytes(), garbage, zero_head=256)
    for B, ncell in ((2, 9 * 157 * 209), (1, 63)):
        logit, res, tgt = (rng.standard_normal((B, 2, ncell)).astype(np.float32), rng.standard_normal((B, 3, ncell)).astype(np.float32),
                           rng.standard_normal((B, 3, ncell)).astype(np.float32))
        pos, cm, rm = [(rng.random((B, ncell)) < q).astype(np.uint8) for q in (0.1, 0.4, 0.1)]
        cw, rw = rng.random((B, ncell)).astype(np.float32), rng.random((B, ncell)).astype(np.float32)
        args = (T(logit).data_ptr(), T(res).data_ptr(), T(tgt).data_ptr(), T(pos).data_ptr(), T(cm).data_ptr(), T(cw).data_ptr(),
                T(rm).data_ptr(), T(rw).data_ptr(), B, ncell, 0.11)
        l, r, cls, reg = _occ_loss_ref(logit, res, tgt, pos, cm, cw, rm, rw, 0.11, 1.0, 0.1)
        out2, n2, out3, n3 = G((2,), "float32"), G((2,), "float32"), G((3,), "float32"), G((2,), "float32")
        ac.call("btc_occ_loss_fwd", *args, 1.0, 0.1, out2.ptr, n2.ptr, ws.ptr, ws.ws_bytes)
        assert ws.head_zero()
        ac.call("btc_occ_loss_fwd_total", *args, 1.0, 0.1, out3.ptr, n3.ptr, ws.ptr, ws.ws_bytes)
        assert ws.head_zero()
        np.testing.assert_allclose(H(out2), [float(cls.detach()), float(reg.detach())], rtol=2e-6)
        assert torch.equal(out3.tensor[:2], out2.tensor) and torch.equal(n3.tensor, n2.tensor)
        assert float(H(out3)[2]) == float(np.float32(H(out2)[0] + H(out2)[1]))
        (0.7 * (cls + reg)).backward()
        g2 = torch.tensor([0.7, 0.7], device=DEV)
        dl2, dr2 = G((B, 2, ncell), "float32"), G((B, 3, ncell), "float32")
        dl2.tensor.zero_()
        dr2.tensor.zero_()                       # the two-scalar form: zero-filled by the caller (header)
        ac.call("btc_occ_loss_bwd", *args, n2.ptr, g2.data_ptr(), dl2.ptr, dr2.ptr)
        dl3, dr3 = G((B, 2, ncell), "float32"), G((B, 3, ncell), "float32")   # the total form writes every cell: poison stays poison
        ac.call("btc_occ_loss_bwd_total", *args, n3.ptr, keep(g2[:1].contiguous()).data_ptr(), dl3.ptr, dr3.ptr)
        assert torch.equal(dl3.tensor, dl2.tensor) and torch.equal(dr3.tensor, dr2.tensor)
        for got, ref in ((H(dl3), l.grad.numpy()), (H(dr3), r.grad.numpy())):
            assert np.abs(got - ref).max() <= 2e-5 * (np.abs(ref).max() + 1e-30)


def case_vfe(garbage):
    from oracle import occ_oracle
    rng = np.random.default_rng(23)
    for M, P in ((2049, 12), (1, 5)):
        C = 6
        num = rng.integers(0, P + 1, M).astype(np.int32)
        vox = rng.standard_normal((M, P, C)).astype(np.float32)
        for i in range(M):
            vox[i, num[i]:] = 0
        for isf in (0, 1):
            n = num.astype(np.float32) if isf else num
            out = G((M, C), "float32")
            ac.call("btc_mean_vfe", T(vox).data_ptr(), T(n).data_ptr(), isf, M, P, C, out.ptr)
            ref = occ_oracle.mean_vfe(torch.from_numpy(vox), torch.from_numpy(num)).numpy()
            np.testing.assert_allclose(H(out), ref, rtol=1e-6, atol=1e-6)
        F_, R = 6, 4
        vox[:, :, 5] = np.where(rng.random((M, P)) < 0.3, 0.5, 0.0)
        feat, occ = G((M, F_), "float32"), G((M, F_ - R), "float32")
        ac.call("btc_occ_vfe", T(vox).data_ptr(), T(num).data_ptr(), 0, M, P, F_, R, feat.ptr, occ.ptr)
        rf = occ_oracle.occ_vfe(torch.from_numpy(vox), torch.from_numpy(num), n_raw=R)
        rf = rf[0] if isinstance(rf, tuple) else rf
        np.testing.assert_allclose(H(feat), rf.numpy(), rtol=1e-6, atol=1e-6)
        np.testing.assert_array_equal(H(occ), H(feat)[:, R:])


# ============================================================================================================ PassOccVox, revoxelize
def _pov_topk(p, thr, max_k):
    """per scene: cells with p > thr, the max_k largest (ties at the cut towards lower cell ids), in ascending cell order"""
    sel = []
    for b in range(p.shape[0]):
        q = p[b].reshape(-1)
        cand = np.nonzero(q > thr)[0]
        order = np.lexsort((cand, -q[cand]))          # descending probability, then ascending cell id
        sel.append(np.sort(cand[order[:max_k]]))
    return sel


def case_pass_occ_vox(garbage):
    from btcdet_amd._lib import BtcPovConfig
    rng = np.random.default_rng(24)
    geoms = [(2, 300, 40), (1, 7, 17)]
    def cfg_for(B, max_k):
        c = BtcPovConfig()
        c.batch, c.max_k = B, max_k
        c.occ_grid[:], c.det_grid[:] = [40, 30, 5], [80, 60, 10]
        c.occ_origin[:], c.occ_voxel[:] = [0.0, -30.0, -2.0], [1.0, 2.0, 1.0]
        c.det_origin[:], c.det_voxel[:] = [0.0, -30.0, -3.0], [0.5, 1.0, 0.5]
        c.occ_thresh, c.inten, c.code_dim = 0.5, 0.0, 2
        return c
    P, C = 3, 4
    wsb = max(L().btc_pass_occ_vox_ws_bytes(ctypes.byref(cfg_for(B, k)), M, P) for B, k, M in geoms)
    ws = W(wsb, garbage)
    for B, max_k, M in geoms:
        c = cfg_for(B, max_k)
        probs = (np.round(rng.random((B, 5, 30, 40)) * 64) / 64).astype(np.float32)
        lin = np.sort(rng.choice(B * 10 * 60 * 80, M, replace=False))
        b, r = lin // 48000, lin % 48000
        dc = np.stack([b, r // 4800, (r // 80) % 60, r % 80], 1).astype(np.int32)
        dn = rng.integers(1, P + 1, M).astype(np.int32)
        dv = rng.standard_normal((M, P, C)).astype(np.float32)
        info = G((2 + B,), "int32")
        ac.call("btc_pass_occ_vox_count", ctypes.byref(c), T(probs).data_ptr(), None, None, None, T(dc).data_ptr(), T(dn).data_ptr(), M, P, C,
                info.ptr, ws.ptr, ws.ws_bytes)
        inf = H(info)
        sel = _pov_topk(probs, 0.5, max_k)
        assert list(inf[2:]) == [len(s) for s in sel]
        m, pmax, k = int(inf[0]), int(inf[1]), int(sum(inf[2:]))
        for i32 in (True, False):
            vox, vc, vn, op, ob = G((m, pmax, C + 2), "float32"), G((m, 4), "int64"), G((m,), "int64"), G((k, 4), "float32"), G((k,), "int64")
            vc32, vn32 = G((m, 4), "int32"), G((m,), "int32")
            if i32:
                ac.call("btc_pass_occ_vox_fill_i32", ctypes.byref(c), T(dv).data_ptr(), M, P, C, m, pmax, k, vox.ptr, vc.ptr, vn.ptr, op.ptr, ob.ptr,
                        vc32.ptr, vn32.ptr, ws.ptr, ws.ws_bytes)
                np.testing.assert_array_equal(H(vc32), H(vc))
                np.testing.assert_array_equal(H(vn32), H(vn))
            else:
                ac.call("btc_pass_occ_vox_fill", ctypes.byref(c), T(dv).data_ptr(), M, P, C, m, pmax, k, vox.ptr, vc.ptr, vn.ptr, op.ptr, ob.ptr,
                        ws.ptr, ws.ws_bytes)
                np.testing.assert_array_equal(H(vc), ref_vc)
                np.testing.assert_array_equal(H(vn), ref_vn)
                np.testing.assert_array_equal(H(vox), ref_vox)
            np.testing.assert_array_equal(H(ob), np.concatenate([np.full(len(s), i) for i, s in enumerate(sel)]).astype(np.int64))
            np.testing.assert_array_equal(H(op)[:, 3], np.concatenate([probs[i].reshape(-1)[s] for i, s in enumerate(sel)]))
            assert np.isfinite(H(op)).all() and np.isfinite(H(vox)).all()
            v = H(vc)
            assert np.all(np.diff(v[:, 0] * (1 << 40) + v[:, 1] * (1 << 30) + v[:, 2] * (1 << 15) + v[:, 3]) > 0), "not sorted unique"
            assert int(H(vn).sum()) == int(dn.sum()) + k
            ref_vc, ref_vn, ref_vox = H(vc), H(vn), H(vox)


def case_revoxelize(garbage):
    rng = np.random.default_rng(25)
    B, shape, C = 2, (40, 160, 140), 6
    ns = (5001, 65, 1)
    ws = W(max(L().btc_revoxelize_ws_bytes(n, B, i3p(shape)) for n in ns), garbage)
    for n in ns:
        coords = np.stack([rng.integers(0, B, n), rng.integers(0, 4, n), rng.integers(0, 30, n), rng.integers(0, 30, n)], 1).astype(np.int64)
        pts = rng.standard_normal((n, C)).astype(np.float32)
        mp = G((2,), "int32")
        tc = T(coords)
        ac.call("btc_revoxelize_count", tc.data_ptr(), n, B, i3p(shape), mp.ptr, mp.ptr + 4, ws.ptr, ws.ws_bytes)
        m, pmax = (int(v) for v in H(mp))
        rv, rnum, rvc = orc.revoxelize(pts, coords)
        assert (m, pmax) == (rv.shape[0], rv.shape[1])
        v, vc, vn = G((m, pmax, C), "float32"), G((m, 4), "int64"), G((m,), "int64")
        ac.call("btc_revoxelize_fill", T(pts).data_ptr(), tc.data_ptr(), n, C, B, i3p(shape), m, pmax, v.ptr, vc.ptr, vn.ptr, ws.ptr, ws.ws_bytes)
        np.testing.assert_array_equal(H(vc), rvc)
        np.testing.assert_array_equal(H(vn), rnum)
        np.testing.assert_array_equal(H(v), rv)


# ============================================================================================================ heads
def _boxes(rng, n):
    return np.concatenate([rng.uniform(-10, 10, (n, 3)), rng.uniform(1, 4, (n, 3)), rng.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)


def case_boxes_nms(garbage):
    rng = np.random.default_rng(26)
    for na, nb in ((65, 129), (1, 17)):
        a, b = _boxes(rng, na), _boxes(rng, nb)
        for mode in (0, 1):
            out = G((na, nb), "float32")
            ac.call("btc_boxes_pairwise_bev", T(a).data_ptr(), na, T(b).data_ptr(), nb, mode, out.ptr)
            ref = orc.boxes_overlap_bev(a, b, iou=bool(mode))
            np.testing.assert_allclose(H(out), ref, rtol=1e-4, atol=(2e-5 if mode else 1e-4))
    for n in (1025, 63, 1):
        bx = _boxes(rng, n)
        bx[:, :2] *= 0.3                                 # crowded: plenty of suppression
        scores = rng.random(n).astype(np.float32)
        order = np.argsort(-scores, kind="stable")
        sb = np.ascontiguousarray(bx[order])
        ref = orc.nms(sb, -np.arange(n, dtype=np.float32), 0.2)       # (already sorted: identity order)
        ws = W(L().btc_nms_ws_bytes(n), garbage)
        keep, nk = G((n,), "int64"), G((1,), "int32")
        ac.call("btc_nms", T(sb).data_ptr(), n, 0.2, 1, keep.ptr, nk.ptr, ws.ptr, ws.ws_bytes)
        k = int(H(nk)[0])
        np.testing.assert_array_equal(H(keep)[:k], ref)
        still_poison(keep, slice(k, None))
        for batch, max_keep in ((3, 7), (1, n + 3)):
            boxes = np.stack([sb] * batch)
            wt = W(L().btc_nms_topk_ws_bytes(batch, n, max_keep), garbage)
            kt, nkt = G((batch, max_keep), "int64"), G((batch,), "int32")
            ac.call("btc_nms_topk", T(boxes).data_ptr(), batch, n, 0.2, 1, max_keep, kt.ptr, nkt.ptr, wt.ptr, wt.ws_bytes)
            r = ref[:max_keep]
            for bb in range(batch):
                assert int(H(nkt)[bb]) == len(r)
                np.testing.assert_array_equal(H(kt)[bb, :len(r)], r)
                assert np.all(H(kt)[bb, len(r):] == -1)


def case_ball_group(garbage):
    rng = np.random.default_rng(27)
    for cnt, ncnt, ns, C in (([1500, 700], [130, 65], 16, 35), ([1], [1], 3, 1)):
        xyz = rng.uniform(0, 4, (sum(cnt), 3)).astype(np.float32)
        new = rng.uniform(0, 4, (sum(ncnt), 3)).astype(np.float32)
        M = len(new)
        idx = G((M, ns), "int32")
        ac.call("btc_ball_query", T(new).data_ptr(), T(np.int32(ncnt)).data_ptr(), T(xyz).data_ptr(), T(np.int32(cnt)).data_ptr(), len(cnt), M,
                -1.0, 0.4, ns, idx.ptr)
        ridx, empty = orc.ball_query(0.4, ns, xyz, cnt, new, ncnt)
        got = H(idx).copy()
        assert np.array_equal(got[:, 0] == -1, empty)
        got[empty] = 0
        np.testing.assert_array_equal(got, ridx)
        feat = rng.standard_normal((sum(cnt), C)).astype(np.float32)
        out = G((M, C, ns), "float32")
        ac.call("btc_group_points", T(feat).data_ptr(), T(np.int32(cnt)).data_ptr(), T(ridx).data_ptr(), T(np.int32(ncnt)).data_ptr(),
                len(cnt), M, C, ns, out.ptr)
        np.testing.assert_array_equal(H(out), orc.group_points(feat, cnt, ridx, ncnt))
        go = rng.standard_normal((M, C, ns)).astype(np.float32)
        gf = G((sum(cnt), C), "float32")           # zeroed by the call (header)
        ac.call("btc_group_points_grad", T(go).data_ptr(), T(ridx).data_ptr(), T(np.int32(ncnt)).data_ptr(), T(np.int32(cnt)).data_ptr(),
                len(cnt), M, C, sum(cnt), ns, gf.ptr)
        ref = orc.group_points_grad(go, ridx, ncnt, cnt, sum(cnt))
        np.testing.assert_allclose(H(gf), ref, rtol=1e-5, atol=1e-5)     # fp32 atomics


def case_fps(garbage):
    rng = np.random.default_rng(28)
    for B, N, npoint in ((2, 4097, 256), (1, 1, 1), (3, 65, 17)):
        xyz = rng.uniform(0, 10, (B, N, 3)).astype(np.float32)
        xyz[:, N // 2:] = np.round(xyz[:, N // 2:])        # ties
        temp = G((B, N), "float32")
        temp.tensor.fill_(1e10)
        idx = G((B, npoint), "int32")
        ac.call("btc_furthest_point_sampling", T(xyz).data_ptr(), B, N, npoint, temp.ptr, idx.ptr)
        np.testing.assert_array_equal(H(idx), orc.furthest_point_sample(xyz, npoint))


def case_three_nn_interp(garbage):
    rng = np.random.default_rng(29)
    for uc, kc, C in (([1025, 63], [300, 17], 32), ([1], [3], 1)):
        u = rng.uniform(0, 5, (sum(uc), 3)).astype(np.float32)
        k = rng.uniform(0, 5, (sum(kc), 3)).astype(np.float32)
        N = len(u)
        d2, idx = G((N, 3), "float32"), G((N, 3), "int32")
        ac.call("btc_three_nn", T(u).data_ptr(), T(np.int32(uc)).data_ptr(), T(k).data_ptr(), T(np.int32(kc)).data_ptr(), len(uc), N, d2.ptr, idx.ptr)
        rd, ri = orc.three_nn(u, uc, k, kc)
        np.testing.assert_array_equal(H(idx), ri)
        np.testing.assert_array_equal(np.sqrt(H(d2)), rd)
        w = rng.random((N, 3)).astype(np.float32)
        feat = rng.standard_normal((sum(kc), C)).astype(np.float32)
        out = G((N, C), "float32")
        ac.call("btc_three_interpolate", T(feat).data_ptr(), T(ri).data_ptr(), T(w).data_ptr(), N, C, out.ptr)
        np.testing.assert_allclose(H(out), orc.three_interpolate(feat, ri, w), rtol=1e-6, atol=1e-6)
        go = rng.standard_normal((N, C)).astype(np.float32)
        gf = G((sum(kc), C), "float32")
        ac.call("btc_three_interpolate_grad", T(go).data_ptr(), T(ri).data_ptr(), T(w).data_ptr(), N, C, sum(kc), gf.ptr)
        ref = np.zeros((sum(kc), C))
        np.add.at(ref, ri.reshape(-1), (go[:, None, :].astype(np.float64) * w[:, :, None]).reshape(-1, C))
        np.testing.assert_allclose(H(gf), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())     # fp32 atomics vs float64


def case_trilinear(garbage):
    from btcdet_amd import conv_head, spconv
    g = torch.Generator().manual_seed(30)
    rng_, vs, stride, B, C = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0], [0.05, 0.05, 0.1], [8.0, 8.0, 8.0], 2, 16
    shape = [5, 200, 176]
    for n_vox, Q in ((3000, 4097), (1, 65)):
        cells = torch.stack([torch.randint(0, B, (n_vox,), generator=g), torch.randint(0, 5, (n_vox,), generator=g),
                             torch.randint(60, 140, (n_vox,), generator=g), torch.randint(40, 130, (n_vox,), generator=g)], 1)
        cells = torch.unique(cells, dim=0).int()
        N = cells.shape[0]
        feats = torch.relu(torch.randn(N, C, generator=g)).to(DEV)
        pts = torch.stack([torch.rand(Q, generator=g) * 40.0 + 14.0, torch.rand(Q, generator=g) * 36.0 - 18.0,
                           torch.rand(Q, generator=g) * 5.0 - 3.5], 1).to(DEV)
        ppb = (Q + 1) // 2
        idx = cells.long().to(DEV)
        live = (feats != 0).any(1).to(torch.uint8)
        cell_row = torch.full((B,) + tuple(shape), -1, dtype=torch.int32, device=DEV)
        cell_row[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = torch.arange(N, dtype=torch.int32, device=DEV)
        rows, wts, flag = G((Q, 8), "int32"), G((Q, 8), "float32"), G((Q,), "uint8")
        f3, i3 = ctypes.c_float * 3, ctypes.c_int32 * 3
        ac.call("btc_trilinear_corners", pts.data_ptr(), Q, ppb, f3(*rng_[:3]), f3(*vs), f3(*stride), i3(*shape), B, cell_row.data_ptr(),
                live.data_ptr(), rows.ptr, wts.ptr, flag.ptr)
        # the dense formulation (itself pinned to the reference's ConvHead) at every point
        x = spconv.SparseConvTensor(feats, cells.to(DEV), shape, B)
        zyx = torch.stack([(pts[:, 2] - rng_[2]) / vs[2] / stride[0] - 0.5, (pts[:, 1] - rng_[1]) / vs[1] / stride[1] - 0.5,
                           (pts[:, 0] - rng_[0]) / vs[0] / stride[2] - 0.5], dim=-1)
        bidx = torch.clamp(torch.arange(Q, device=DEV) // ppb, max=B - 1)
        ref = conv_head.trilinear_readout(x, bidx, zyx)
        assert torch.equal(flag.tensor.bool(), (ref.abs() > 0).any(-1))
        r, w = rows.tensor, wts.tensor
        assert bool(((r >= -1) & (r < N)).all()) and bool((w[r < 0] == 0).all())
        kept = torch.nonzero(flag.tensor)[:, 0]
        M = kept.numel()
        rk, wk = r[kept].contiguous(), w[kept].contiguous()
        out = G((M, C), "float32")
        ac.call("btc_trilinear_gather", feats.data_ptr(), C, M, rk.data_ptr(), wk.data_ptr(), out.ptr)
        assert torch.equal(out.tensor, ref[kept])
        grad = torch.randn((M, C), generator=g).to(DEV)
        key = torch.where((rk >= 0) & (wk != 0), rk, torch.full_like(rk, N)).view(-1)
        skey, perm = torch.sort(key, stable=True)
        seg = torch.searchsorted(skey, torch.arange(N + 1, dtype=skey.dtype, device=DEV)).int()
        gf = G((N, C), "float32")
        ac.call("btc_trilinear_scatter", grad.data_ptr(), C, keep(perm.int()).data_ptr(), seg.data_ptr(), wk.data_ptr(), N, gf.ptr)
        ref_g = torch.zeros((N, C), dtype=torch.float64, device=DEV)
        e = torch.nonzero(key < N)[:, 0]
        ref_g.index_add_(0, key[e].long(), grad.double()[e // 8] * wk.view(-1).double()[e][:, None])
        assert float((gf.tensor.double() - ref_g).abs().max()) <= 2e-6 * (float(ref_g.abs().max()) + 1e-30)


# ============================================================================================================ optimizer
def case_adam(garbage):
    rng = np.random.default_rng(31)
    maxseg = L().btc_adam_max_segments()
    for sizes in ((1500, 37, 2049), (1,)):
        grads = [T(rng.standard_normal(s).astype(np.float32) * 0.3) for s in sizes]
        seg, off, ln, flat_off, chunk0 = [], [], [], [], []
        base = 0
        for s, n in enumerate(sizes):
            chunk0.append(len(seg))
            for o in range(0, n, 1024):
                seg.append(s % maxseg)
                off.append(o)
                ln.append(min(1024, n - o))
                flat_off.append(base + o)
            base += n
        chunk0.append(len(seg))
        nt = base
        gp = (ctypes.c_void_p * len(sizes))(*[t.data_ptr() for t in grads])
        tabs = (T(np.int32(seg)), T(np.int32(off)), T(np.int32(ln)), T(np.int64(flat_off)))
        c0 = np.array(chunk0, np.int32)
        flat = G((nt,), "float32")
        ac.call("btc_grads_pack", gp, len(sizes), *[t.data_ptr() for t in tabs], c0.ctypes.data_as(c_i32p), flat.ptr)
        g64 = np.concatenate([t.cpu().numpy() for t in grads]).astype(np.float64)
        np.testing.assert_array_equal(H(flat), g64.astype(np.float32))
        p0 = rng.standard_normal(nt).astype(np.float32)
        m0 = rng.standard_normal(nt).astype(np.float32) * 0.01
        v0 = rng.random(nt).astype(np.float32) * 0.01
        p, m, v = T(p0), T(m0), T(v0)
        ws = W(L().btc_adam_group_ws_bytes(len(seg)), garbage)
        lr, b1, b2, eps, wd, clip, step = 0.003, 0.9, 0.99, 1e-8, 0.01, 0.5, 3
        ac.call("btc_adam_group_step", gp, len(sizes), *[t.data_ptr() for t in tabs], c0.ctypes.data_as(c_i32p), len(seg), p.data_ptr(),
                m.data_ptr(), v.data_ptr(), step, lr, b1, b2, eps, wd, clip, ws.ptr, ws.ws_bytes)
        sq = float(ws.tensor[:8].cpu().numpy().view(np.float64)[0])
        assert abs(sq - float((g64 ** 2).sum())) <= 1e-6 * float((g64 ** 2).sum())
        coef = 1.0 / max(1.0, (np.sqrt((g64 ** 2).sum()) + 1e-6) / clip)
        g = g64 * coef
        pr = p0.astype(np.float64) * (1 - wd * lr)
        mr = m0 + (g - m0) * (1 - b1)
        vr = b2 * v0 + (1 - b2) * g * g
        pr = pr - lr / (1 - b1 ** step) * mr / (np.sqrt(vr) / np.sqrt(1 - b2 ** step) + eps)
        np.testing.assert_allclose(p.cpu().numpy(), pr, rtol=2e-5, atol=2e-7)
        np.testing.assert_allclose(m.cpu().numpy(), mr, rtol=2e-5, atol=2e-6 * np.abs(mr).max())
        np.testing.assert_allclose(v.cpu().numpy(), vr, rtol=2e-5, atol=2e-6 * np.abs(vr).max())


# ============================================================================================================ poisoned allocations
import contextlib  # noqa: E402


@contextlib.contextmanager
def poisoned_allocations():
    """torch.empty / empty_like / Tensor.new_empty return memory filled with the poison of their dtype (device tensors only)"""
    count = [0]
    e, el, ne = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def _p(t):
        if t.is_cuda and t.numel() and ac._dname(t.dtype) in ac.POISON:
            count[0] += 1
            ac.poison_like(t)
        return t

    def empty(*a, **k):
        return _p(e(*a, **k))

    def empty_like(*a, **k):
        return _p(el(*a, **k))

    def new_empty(self, *a, **k):
        return _p(ne(self, *a, **k))

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    try:
        yield count
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = e, el, ne


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_poisoned_allocations_leave_the_training_step_bit_identical(dtype):
    import bench
    from btcdet_amd.btc_path import BtcHotPath
    from btcdet_amd.config import load_cfg
    d = torch.device(DEV)
    batch = bench.build_batches(1, 0, d)[0]
    cfg = load_cfg()
    cfg.MODEL.OCC.BACKBONE_3D["FEATURE_DTYPE"] = dtype
    cfg.MODEL.BACKBONE_3D["FEATURE_DTYPE"] = dtype
    torch.manual_seed(0)
    np.random.seed(0)
    model = BtcHotPath(cfg, device=d).to(d).train()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    rng_state = (np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state(d))

    def step():
        np.random.set_state(rng_state[0])
        torch.set_rng_state(rng_state[1])
        torch.cuda.set_rng_state(rng_state[2], d)
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        bd = model.dataset.data_processor.forward_batch(batch["points"], batch["pre_rot_points"], batch["scene_offsets"], batch["rot_z"])
        bd.update({"batch_size": 2, "points": batch["points5"], "gt_boxes": batch["gt_boxes"], "gt_boxes_num": batch["gt_boxes_num"],
                   "box_mirr_flag": batch["box_mirr_flag"], "bm_points": batch["bm_points"], "rot_z": batch["rot_z"], "is_train": True})
        ret, _, _ = model(bd)
        loss = ret["loss_occ"] + 1e-3 * ret["spatial_features"].float().pow(2).mean() + 1e-3 * ret["x_combine"].float().pow(2).mean()
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        bufs = {n: b.detach().clone() for n, b in model.named_buffers()}
        return loss.detach().clone(), grads, bufs

    l0, g0, b0 = step()
    with poisoned_allocations() as count:
        l1, g1, b1 = step()
    assert count[0] > 0, "the patch was not reached"
    assert torch.equal(l0, l1), (float(l0), float(l1))
    assert set(g0) == set(g1) and len(g0) > 0
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    for n in b0:
        assert torch.equal(b0[n], b1[n]), n
