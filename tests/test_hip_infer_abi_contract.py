"""The buffer contract of the entry points of include/btcdet_hip_infer.h, as tests/test_hip_abi_contract.py holds the first header to it:
every output is a Guarded buffer (poisoned payload between two guard bands), every workspace the library may use is garbage.  After
a call the poisoned y is fully overwritten, the guards are intact, and the read-only inputs -- the running statistics above all --
hold the bits they held before."""
import numpy as np
import pytest
import torch

import abi_contract as ac
from test_hip_conv_kernel_volumes import SPLIT_Z, Case, L, _g, _split_planes, tuned

pytestmark = pytest.mark.gpu

EPS = 1e-3


def _call_on_stream(stream, fn, *args):
    torch.cuda.current_stream().synchronize()
    rc = fn(*args, stream.cuda_stream)
    stream.synchronize()
    assert rc == 0, "rc %d: %s" % (rc, L().btc_last_error().decode("utf-8", "replace"))


# (operands, K, n, cin, cout, z-split key): every operand kind; fp32 through conv_apply_g, conv_apply and conv_apply_ws; the split kernel with
# its own epilogue and with split_reduce's (z-split through a garbage scratch buffer)
CONTRACT = [(0, 27, 2049, 16, 32, 0), (0, 8, 63, 6, 18, 0), (0, 12, 4097, 4, 16, 0), (0, 3, 1, 16, 16, 0), (1, 27, 1601, 32, 64, 0), (2, 12, 129, 64, 48, 0),
            (3, 27, 3000, 64, 64, 1), (3, 12, 3000, 128, 128, 4), (3, 16, 999, 64, 64, 2)]


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
@pytest.mark.parametrize("operands,K,n,cin,cout,z", CONTRACT)
def test_conv_bn_eval_fwd_buffer_contract(operands, K, n, cin, cout, z, garbage):
    from btcdet_amd._lib import check, ptr, stream_ptr
    bf = operands in (1, 2)
    c = Case(K + n + operands, n, K, cin, cout, bf16=bf, pairs_per_row=5.0)
    rng = np.random.default_rng(n)
    gamma, beta = _g(rng.uniform(0.5, 1.5, cout).astype(np.float32)), _g(rng.uniform(-0.5, 0.5, cout).astype(np.float32))
    rm, rv = _g(rng.uniform(-0.3, 0.3, cout).astype(np.float32)), _g(rng.uniform(0.3, 1.7, cout).astype(np.float32))
    W = c.w
    if operands == 2:
        q = torch.empty((2, c.w.numel()), dtype=torch.bfloat16, device=c.w.device)
        check(L().btc_weights_to_bf16(ptr(c.w), K, cin, cout, ptr(q[0]), ptr(q[1]), stream_ptr()), "btc_weights_to_bf16")
        W = q[1]
    elif operands == 3:
        W = _split_planes(c)[1]
    inputs = [c.f, W, c.b, c.m_out, c.o, gamma, beta, rm, rv]
    before = [t.clone() for t in inputs]
    s = torch.cuda.Stream()
    scratch = ac.Workspace(16 << 20, garbage=garbage)          # the stream's scratch buffer: z-split launches write their slabs there
    check(L().btc_set_scratch(s.cuda_stream, scratch.ptr, scratch.ws_bytes), "btc_set_scratch")
    try:
        y = ac.Guarded((n, cout), "bfloat16" if bf else "float32")
        assert bool(y.poison_mask().all())
        with tuned((SPLIT_Z, z)):
            _call_on_stream(s, L().btc_conv_bn_eval_fwd, operands, ptr(c.f), c.f.shape[0], ptr(W), ptr(c.b), ptr(c.m_out), ptr(c.o), n, K, cin, cout,
                            ptr(gamma), ptr(beta), ptr(rm), ptr(rv), EPS, 1, y.ptr)
        assert not bool(y.poison_mask().any()), "%d of %d elements of y left as poison" % (int(y.poison_mask().sum()), y.tensor.numel())
        assert y.guards_intact() and scratch.guards_intact()
        assert bool(torch.isfinite(y.tensor.float()).all()) and float(y.tensor.float().min()) >= 0.0
        for t, b in zip(inputs, before):
            assert torch.equal(t, b), "an input was written"
        # the same call on the current stream (its own scratch, no guards) gives the same bits
        y2 = torch.empty_like(y.tensor)
        with tuned((SPLIT_Z, z)):
            if operands == 3:
                from test_hip_conv_kernel_volumes import _ensure_scratch
                _ensure_scratch()
            check(L().btc_conv_bn_eval_fwd(operands, ptr(c.f), c.f.shape[0], ptr(W), ptr(c.b), ptr(c.m_out), ptr(c.o), n, K, cin, cout, ptr(gamma),
                                           ptr(beta), ptr(rm), ptr(rv), EPS, 1, ptr(y2), stream_ptr()), "btc_conv_bn_eval_fwd")
            torch.cuda.synchronize()
        assert torch.equal(y2, y.tensor)
    finally:
        check(L().btc_set_scratch(s.cuda_stream, None, 0), "btc_set_scratch")


def test_nothing_is_written_when_the_arguments_are_refused():
    """an argument error leaves y as it was"""
    from btcdet_amd._lib import ptr, stream_ptr
    c = Case(9, 70, 27, 16, 16)
    rm, rv = torch.zeros(16, device=c.w.device), torch.ones(16, device=c.w.device)
    y = ac.Guarded((70, 16), "float32")
    for kw in (dict(n=0), dict(operands=5), dict(rm=None)):
        rc = L().btc_conv_bn_eval_fwd(kw.get("operands", 0), ptr(c.f), c.f.shape[0], ptr(c.w), None, ptr(c.m_out), None, kw.get("n", 70), 27, 16, 16, None, None,
                                      ptr(rm) if "rm" not in kw else None, ptr(rv), EPS, 1, y.ptr, stream_ptr())
        assert rc == -1, kw
    torch.cuda.synchronize()
    assert bool(y.poison_mask().all()) and y.guards_intact()
