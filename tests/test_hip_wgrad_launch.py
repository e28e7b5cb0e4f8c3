"""Every weight-gradient family launches what its plan says (csrc/conv_wgrad.h WgradLaunch: the instance, its grid, its LDS bytes and the
slab count the workspace was checked against), through the C ABI on the synthetic maps of tests/test_hip_conv_kernel_volumes.py.

Per case, in fp32 and bf16, with dW and the workspace NaN-filled before the call:
  (i)   btc_conv_wgrad_slabs reports 1 <= n_slabs and n_slabs K Cin Cout floats fit in btc_conv_wgrad_ws_bytes -- a launch that writes
        more slabs than were planned, or a planner that sizes for fewer, fails here or leaves NaN in (ii);
  (ii)  the one-call form and the two-call form + btc_wgrad_reduce_multi give identical bits;
  (iii) the suite's bars against float64 hold: 1e-4 of the scale for fp32 (_wgrad_bar), 4e-6 of the scale for bf16 activations against
        float64 over the same bf16-rounded inputs (tests/test_hip_wgrad_x.py).
The shapes are the smallest that reach each family (thresholds of wgrad_plan_rows, btc_wgrad_x_plan and wgrad_choose).  Where the bf16-pipe
or the narrow family is meant to run, its bits differ from the run with the family's key off; the four fp32-pipe families add the same
products in the same order and have no such observable -- for them (i)-(iii) on shapes only they are given is the check."""
import ctypes

import numpy as np
import pytest
import torch

from test_hip_conv_kernel_volumes import NARROW, WGRAD_PIPE, WGRAD_X, X_DEPTH, Case, L, _g, _wgrad_bar, tuned
from test_hip_core import dev
from test_hip_wgrad_x import _x_shape

pytestmark = pytest.mark.gpu

FP32_PIPE = ((WGRAD_X, 1), (NARROW, 1))
# (family, cin, cout, K, rows, keys)
LAUNCH_CASES = [
    ("rows_p", 16, 16, 3, 4096, FP32_PIPE), ("rows_p", 16, 16, 3, 4160, FP32_PIPE), ("rows_p", 16, 16, 3, 4161, FP32_PIPE),
    ("rows", 16, 16, 3, 4096, FP32_PIPE + ((WGRAD_PIPE, 1),)), ("rows", 16, 16, 3, 4160, FP32_PIPE + ((WGRAD_PIPE, 1),)),
    ("rows", 16, 16, 3, 4161, FP32_PIPE + ((WGRAD_PIPE, 1),)),
    ("partial_p", 16, 16, 65, 129, FP32_PIPE), ("partial", 16, 16, 65, 129, FP32_PIPE + ((WGRAD_PIPE, 1),)),
    ("partial_scalar", 34, 32, 3, 129, FP32_PIPE),
    ("x", 16, 16, 3, 2048, ((NARROW, 1),)), ("x", 32, 16, 3, 2048, ((NARROW, 1),)),
    ("x_full_ph", 16, 16, 27, 49152, ((NARROW, 1),)), ("x_full_ph", 32, 32, 27, 49152, ((NARROW, 1),)),
    ("x_swapped", 64, 32, 3, 16384, ((NARROW, 1),)),
    ("n_result_mirrored", 32, 5, 3, 2048, ()), ("n_result", 32, 5, 3, 2048, ()), ("n_input", 4, 16, 3, 2048, ()),
    # paths of the fp32-pipe kernels that no row above reaches (csrc/wgrad_tile.h): two Cin blocks (the second with one live wave of
    # four) x two Cout blocks of NT = 8 (the second 16 columns wide); scalar staging of both operands with the Cout bound inside a
    # 16-column tile; conv_wgrad_rows with scalar / mixed staging (the plan takes it because Cg & 3); conv_wgrad_rows_p with
    # bcol < Cout live; swap = 1 (2 * 4096 < 8200: 4096 walked rows, transposed slab store)
    ("partial_p_blocks", 80, 144, 2, 129, FP32_PIPE), ("partial_blocks", 80, 144, 2, 129, FP32_PIPE + ((WGRAD_PIPE, 1),)),
    ("partial_scalar", 34, 30, 3, 129, FP32_PIPE),
    ("rows_scalar", 30, 30, 3, 4161, FP32_PIPE), ("rows_mixed", 30, 32, 3, 4096, FP32_PIPE), ("rows_p_edge", 32, 30, 3, 4161, FP32_PIPE),
    ("rows_p_swapped", 64, 32, 3, 8200, FP32_PIPE), ("rows_swapped", 64, 32, 3, 8200, FP32_PIPE + ((WGRAD_PIPE, 1),)),
]


def make_case(family, cin, cout, K, rows, bf16):
    """the layer of one LAUNCH_CASES row; n_result_mirrored: a map that is its own transpose with the offset index mirrored
    (nbr_in[j][k] == nbr_out[j][K - 1 - k], K = 3: a partial injection, a partial identity, the injection's inverse), as a submanifold
    rulebook's is, handed in as nbr_in == nbr_out; x_swapped / *_swapped: an input side of rows // 8 / rows // 2 - 4 rows"""
    kw = dict(n_src=rows // 8) if family == "x_swapped" else (dict(n_src=rows // 2 - 4) if family.endswith("_swapped") else {})
    c = Case(cin * 1000 + cout * 10 + K + rows, rows, K, cin, cout, bf16=bf16, pairs_per_row=min(K, 4.0), **kw)
    if family == "n_result_mirrored":
        fwd = c.nbr_out[:, 0]
        inv = np.full(rows, -1, np.int32)
        inv[fwd[fwd >= 0]] = np.nonzero(fwd >= 0)[0]
        mid = np.where(c.nbr_out[:, 1] >= 0, np.arange(rows, dtype=np.int32), -1).astype(np.int32)
        c.nbr_out = np.ascontiguousarray(np.stack([fwd, mid, inv], 1))
        c.nbr_in = np.ascontiguousarray(c.nbr_out[:, ::-1])
        c.m_out, c.m_in = _g(c.nbr_out), _g(c.nbr_in)
    return c


def wgrad_both_forms(c, mirrored=False):
    """-> (dW of the one-call form, dW of btc_conv_wgrad_slabs + btc_wgrad_reduce_multi, n_slabs, workspace bytes)"""
    from btcdet_amd._lib import check, ptr, stream_ptr
    bf = c.f.dtype == torch.bfloat16
    m_in, n_in = (c.m_out, c.n) if mirrored else (c.m_in, c.n_src)
    wsb = L().btc_conv_wgrad_ws_bytes(c.n, c.K, c.cin, c.cout, n_in)
    out = []
    for two_calls in (False, True):
        ws = torch.full((max(wsb, 256) // 4,), float("nan"), device=dev())
        dw = torch.full((c.K, c.cin, c.cout), float("nan"), device=dev())
        n = ctypes.c_int(-1)
        if not two_calls:
            fn = L().btc_conv_wgrad_bf16 if bf else L().btc_conv_wgrad
            check(fn(ptr(c.f), ptr(c.d), ptr(c.m_out), c.n, ptr(m_in), n_in, c.K, c.cin, c.cout, ptr(dw), ptr(ws), wsb, stream_ptr()), "wgrad")
        else:
            check(L().btc_conv_wgrad_slabs(int(bf), ptr(c.f), ptr(c.d), ptr(c.m_out), c.n, ptr(m_in), n_in, None, None, c.K, c.cin, c.cout, ptr(dw),
                                           ptr(ws), wsb, ctypes.byref(n), stream_ptr()), "slabs")
            P, D = (ctypes.c_void_p * 1)(ptr(ws)), (ctypes.c_void_p * 1)(ptr(dw))
            S, C = (ctypes.c_int * 1)(n.value), (ctypes.c_longlong * 1)(dw.numel())
            if n.value >= 1:
                check(L().btc_wgrad_reduce_multi(P, D, S, C, 1, stream_ptr()), "reduce_multi")
        torch.cuda.synchronize()
        out.append(dw)
    return out[0], out[1], n.value, wsb


def _check(c, what, mirrored=False):
    one, two, n_slabs, wsb = wgrad_both_forms(c, mirrored)
    print("%s: %d slabs, %d workspace bytes" % (what, n_slabs, wsb))
    assert 1 <= n_slabs and n_slabs * c.K * c.cin * c.cout * 4 <= wsb, (what, n_slabs, wsb)                # (i)
    assert bool(torch.isfinite(one).all()) and torch.equal(one, two), what + ": the two forms differ"        # (ii)
    ref = c.wgrad64()                                                                                       # (iii)
    if c.f.dtype == torch.bfloat16:
        err, scale = float((one.double() - ref).abs().max()), float(ref.abs().max()) + 1e-12
        print("%s: bf16 max err %.2e of the scale" % (what, err / scale))
        assert err <= 4e-6 * scale, (what, err / scale)
    else:
        _wgrad_bar(one, ref, what)
    return one


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("family,cin,cout,K,rows,keys", LAUNCH_CASES, ids=["%s-%d-%d-%d-%d" % c[:5] for c in LAUNCH_CASES])
def test_every_family_launches_what_was_planned(family, cin, cout, K, rows, keys, bf16):
    c = make_case(family, cin, cout, K, rows, bf16)
    mirrored = family == "n_result_mirrored"
    what = "%s %d->%d K %d %d rows %s" % (family, cin, cout, K, rows, "bf16" if bf16 else "fp32")
    with tuned(*keys):
        got = _check(c, what, mirrored)
    if family.startswith("x"):
        swap = 2 * c.n_src < c.n
        takes = _x_shape(0 if bf16 else 1, cout if swap else cin, cin if swap else cout) is not None
        assert swap == (family == "x_swapped")
        with tuned(*keys, (WGRAD_X, 1)):
            off = wgrad_both_forms(c)[0]
        assert takes == (not torch.equal(got, off)), what + ": the bf16-pipe family " + ("did not run" if takes else "ran")
        for depth in (1, 2):      # items in flight (key 20): the same sums in the same order
            with tuned(*keys, (X_DEPTH, depth)):
                assert torch.equal(_check(c, what + " depth %d" % depth), got), what + ": depth %d" % depth
    if family.startswith("n_"):
        with tuned((NARROW, 1)):
            off = wgrad_both_forms(c, mirrored)[0]
        assert not torch.equal(got, off), what + ": the narrow family did not run"
