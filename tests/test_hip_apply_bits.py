"""The bits of conv_apply_b (bf16 operands) and conv_apply_s (split operands), pinned.

Both kernels are deterministic, but the oracle's bit pattern covers the exact families only: their other tests hold them to float64
bars.  tests/golden/apply_bits.json records, per case, the SHA-1 of the inputs and the SHA-1 of the result bytes as the kernels gave
them when the file was written (tests/golden/gen_apply_bits.py, run on the GPU).  A change that is meant to leave the arithmetic alone
-- moving a prologue or an epilogue, renaming a flag -- keeps every digest; one that is meant to change it regenerates the file and
says so.  The cases are layers on the synthetic maps of tests/test_hip_conv_kernel_volumes.py, forced to an instance with its tune keys;
between them they reach every instance the built-in policy picks (CASES below)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from test_hip_core import dev
from test_hip_conv_kernel_volumes import APPLY_KC, APPLY_NT, BN_FUSE, LOADERS, PAIR, SPLIT_Z, STAGES, Case, L, _ensure_scratch, _g, tuned
from test_hip_eval_fold import EPS, Bn

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "apply_bits.json")
FWD, DGRAD, MIRROR = 0, 1, 2
PLAIN, EVAL, STATS = "plain", "eval", "stats"


def _b(name, n, K, cred, cres, pass_=FWD, order=False, bias=True, pair=1, mode=PLAIN, same_as=None):
    """conv_apply_b: the wave shape follows Cres (16 -> 411, 32 -> 221, 64 -> 141 under 8192 rows and 422 from there, 128 -> 424), the
    reduction chunk Cred (64 | 32, or PAIR with key 21 = 2 on 32 channels and >= 8 offsets)"""
    return dict(name=name, fam="b", n=n, K=K, cred=cred, cres=cres, pass_=pass_, order=order, bias=bias and pass_ == FWD, mode=mode,
                keys=[(PAIR, pair)], same_as=same_as, seed=same_as or name)


def _s(name, shape, kc, n, K, cred, cres, pass_=FWD, order=False, bias=True, pair=1, lw=0, mode=PLAIN, same_as=None):
    """conv_apply_s forced to (wave shape, reduction chunk) with keys 1 and 4, unsplit (key 15 = 1); stages and loader waves are the
    policy's for that pair unless key 17 says otherwise (1 = no loader waves, 2, 4)"""
    keys = [(APPLY_NT, shape), (SPLIT_Z, 1), (PAIR, pair), (LOADERS, lw)]
    if pair != 2:
        keys += [(APPLY_KC, kc), (STAGES, 0)]
    return dict(name=name, fam="s", n=n, K=K, cred=cred, cres=cres, pass_=pass_, order=order, bias=bias and pass_ == FWD, mode=mode,
                keys=keys, same_as=same_as, seed=same_as or name)


# n = 17, 65, 129, 130: a partial last tile at 16, 32, 64 and 128 rows per workgroup; K = 1, 3, 5, 27 (odd: PAIR's tail), 64 (lane 63
# of the offset ballot).  `same_as`: the same inputs through another instance, whose digest must be the same one.
CASES = [
    # ---- conv_apply_b: 5 wave shapes x (PAIR | 32-channel items | 64-channel items)
    _b("b411_pair", 129, 27, 32, 16, pair=2),
    _b("b411_kc32", 129, 27, 32, 16, same_as="b411_pair"),
    _b("b221_pair", 65, 64, 32, 32, DGRAD, order=True, pair=2),
    _b("b221_kc32", 65, 64, 32, 32, DGRAD, order=True, same_as="b221_pair"),
    _b("b141_pair", 17, 27, 32, 64, MIRROR, pair=2),
    _b("b141_kc32", 17, 27, 32, 64, MIRROR, same_as="b141_pair"),
    _b("b422_pair_stats", 8193, 27, 32, 64, pair=2, mode=STATS),
    _b("b422_kc32_stats", 8193, 27, 32, 64, mode=STATS, same_as="b422_pair_stats"),
    _b("b424_pair_eval", 130, 8, 32, 128, pair=2, mode=EVAL),
    _b("b424_kc32_eval", 130, 8, 32, 128, mode=EVAL, same_as="b424_pair_eval"),
    _b("b411_kc64", 17, 1, 64, 48, bias=False),
    _b("b221_kc64", 130, 3, 64, 32, DGRAD),
    _b("b141_kc64", 65, 5, 128, 64, order=True),
    _b("b422_kc64_eval", 8200, 3, 64, 64, order=True, mode=EVAL),
    _b("b424_kc64", 129, 64, 64, 128, MIRROR),
    # ---- conv_apply_s: the (shape, chunk) pairs of btc_apply_split's own choice, with its loader-wave count for each
    _s("s424_kc64", 424, 64, 129, 27, 64, 128, order=True),
    _s("s424_kc32", 424, 32, 65, 3, 96, 128, DGRAD),
    _s("s222_kc64_eval", 222, 64, 65, 64, 64, 64, mode=EVAL),
    _s("s222_kc32", 222, 32, 17, 5, 32, 64, MIRROR),
    _s("s422_kc64", 422, 64, 130, 1, 128, 64, bias=False),
    _s("s422_kc32", 422, 32, 129, 27, 96, 64, DGRAD, order=True),
    _s("s412_kc64_stats", 412, 64, 130, 27, 64, 32, mode=STATS),                              # four loader waves
    _s("s412_kc64_lw2", 412, 64, 130, 27, 64, 32, lw=2, mode=STATS, same_as="s412_kc64_stats"),
    _s("s412_kc64_lw0", 412, 64, 130, 27, 64, 32, lw=1, mode=STATS, same_as="s412_kc64_stats"),
    _s("s412_kc32", 412, 32, 129, 5, 32, 32),                                                  # two loader waves
    _s("s412_kc32_lw0", 412, 32, 129, 5, 32, 32, lw=1, same_as="s412_kc32"),
    _s("s412_pair", 412, 64, 129, 5, 32, 32, pair=2, same_as="s412_kc32"),                     # 5 offsets: a pair and a half
    _s("s812_kc64", 812, 64, 129, 3, 64, 32, MIRROR),
    _s("s812_kc32", 812, 32, 130, 64, 96, 32, order=True),
    # ---- one z-split launch through split_reduce (no keys: 64 x 128 tiles, four workgroups per tile), plain and with the eval epilogue
    dict(name="s_zsplit", fam="s", n=3000, K=12, cred=128, cres=128, pass_=FWD, order=False, bias=True, mode=PLAIN, keys=[], same_as=None,
         seed="s_zsplit"),
    dict(name="s_zsplit_eval", fam="s", n=3000, K=12, cred=128, cres=128, pass_=FWD, order=False, bias=True, mode=EVAL, keys=[], same_as=None,
         seed="s_zsplit"),
]
NAMES = [c["name"] for c in CASES]


def _sha(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _bytes(t):
    return t.contiguous().cpu().view(torch.uint8).numpy()


def _weights(c, fam):
    """-> (dgrad operand, forward operand) of the family, through the single-weight entry points"""
    from btcdet_amd._lib import check, ptr, stream_ptr
    fn, planes = (L().btc_weights_to_bf16, 1) if fam == "b" else (L().btc_weights_split3, 3)
    q = torch.empty((2, planes * c.w.numel()), dtype=torch.bfloat16, device=dev())
    check(fn(ptr(c.w), c.K, c.cin, c.cout, ptr(q[0]), ptr(q[1]), stream_ptr()), "weights")
    return q


def run_case(spec):
    """-> (SHA-1 of the inputs, SHA-1 of the stored result)"""
    from btcdet_amd._lib import check, ptr, stream_ptr
    from btcdet_amd.spconv import fused_bn
    _ensure_scratch()
    fwd = spec["pass_"] == FWD
    cin, cout = (spec["cred"], spec["cres"]) if fwd else (spec["cres"], spec["cred"])
    seed = int(hashlib.sha1(spec["seed"].encode()).hexdigest()[:8], 16)
    c = Case(seed, spec["n"], spec["K"], cin, cout, bf16=spec["fam"] == "b", pairs_per_row=6.0)
    bn = Bn(seed % 1000, cout)
    h_in = _sha(c.nbr_out, c.nbr_in, c.order, c.feat, c.W, c.bias, c.dout, bn.gamma, bn.beta, bn.mean, bn.var)
    q = _weights(c, spec["fam"])
    operands = 2 if spec["fam"] == "b" else 3
    order, bias = spec["order"], spec["bias"]
    with tuned(*spec["keys"]):
        if spec["mode"] == PLAIN and spec["pass_"] != MIRROR:
            out = c.apply(spec["pass_"], operands, W=q[1 - spec["pass_"]], order=order, bias=bias)
        elif spec["mode"] == PLAIN:      # a submanifold layer's dgrad through its forward map: as many source rows as result rows
            out = torch.full((c.n, cin), float("nan"), dtype=c.d.dtype, device=dev())
            check(L().btc_conv_apply_src(MIRROR, operands, ptr(c.d), c.n, ptr(q[0]), None, ptr(c.m_out), ptr(c.o) if order else None, c.n, c.K, cin, cout,
                                         ptr(out), stream_ptr()), "btc_conv_apply_src")
        elif spec["mode"] == EVAL:
            out = torch.full((c.n, cout), float("nan"), dtype=c.f.dtype, device=dev())
            check(L().btc_conv_bn_eval_fwd(operands, ptr(c.f), c.n_src, ptr(q[1]), ptr(c.b) if bias else None, ptr(c.m_out), ptr(c.o) if order else None,
                                           c.n, c.K, cin, cout, ptr(bn.g), ptr(bn.b), ptr(bn.rm), ptr(bn.rv), EPS, 1, ptr(out), stream_ptr()),
                  "btc_conv_bn_eval_fwd")
        else:
            # the statistics epilogue: x is pinned; mean / rstd come from fp64 atomics, so they are held to the separate statistics pass
            # (key 12 = 1) as tests/test_hip_conv_kernel_volumes.py::test_fused_batch_statistics holds them
            runs = []
            for fuse_off in (0, 1):
                x = torch.full((c.n, cout), float("nan"), dtype=c.f.dtype, device=dev())
                y, stats = torch.empty_like(x), torch.empty((2, cout), device=dev())
                rm, rv = torch.zeros(cout, device=dev()), torch.ones(cout, device=dev())
                nbt = torch.zeros((), dtype=torch.long, device=dev())
                need = L().btc_bn_ws_bytes(cout)
                ws = torch.zeros((need,), dtype=torch.uint8, device=dev())
                with tuned((BN_FUSE, fuse_off)):
                    check(L().btc_conv_bn_relu_fwd_src(operands, ptr(c.f), c.n_src, ptr(q[1]), ptr(c.b) if bias else None, ptr(c.m_out),
                                                       ptr(c.o) if order else None, c.n, c.K, cin, cout, ptr(x), ptr(bn.g), ptr(bn.b), ptr(rm), ptr(rv), ptr(nbt),
                                                       0.01, EPS, 1, ptr(y), ptr(stats[0]), ptr(stats[1]), ptr(ws), need, ptr(fused_bn.fuse_ws(dev())),
                                                       stream_ptr()), "btc_conv_bn_relu_fwd_src")
                    torch.cuda.synchronize()
                runs.append((x, stats, rm, rv))
            assert torch.equal(runs[0][0], runs[1][0]), "x with and without the statistics epilogue"
            assert bool((fused_bn.fuse_ws(dev()) == 0).all())
            np.testing.assert_allclose(runs[0][1].cpu().numpy(), runs[1][1].cpu().numpy(), rtol=2e-6, atol=1e-7)
            np.testing.assert_allclose(runs[0][2].cpu().numpy(), runs[1][2].cpu().numpy(), rtol=2e-6, atol=1e-8)
            np.testing.assert_allclose(runs[0][3].cpu().numpy(), runs[1][3].cpu().numpy(), rtol=2e-6, atol=1e-8)
            out = runs[0][0]
        torch.cuda.synchronize()
    assert not bool(out.float().isnan().any()), "a row was never stored"
    return h_in, _sha(_bytes(out))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one(golden):
    assert sorted(golden) == sorted(NAMES)
    for spec in CASES:
        if spec["same_as"]:
            assert golden[spec["name"]]["inputs"] == golden[spec["same_as"]]["inputs"], spec["name"]
            assert golden[spec["name"]]["result"] == golden[spec["same_as"]]["result"], spec["name"]


@pytest.mark.parametrize("name", NAMES)
def test_apply_bits(name, golden):
    h_in, h_out = run_case(CASES[NAMES.index(name)])
    assert h_in == golden[name]["inputs"], "the inputs drifted (Case / synth_map / the generators behind them changed): regenerate the golden file"
    assert h_out == golden[name]["result"], "%s: the result bytes are not the recorded ones" % name


def test_single_weight_conversions_equal_the_multi_forms():
    """btc_weights_to_bf16 / btc_weights_split3 and their _multi forms over two weights of different shape: the same bytes"""
    from btcdet_amd._lib import check, ptr, stream_ptr
    rng = np.random.default_rng(7)
    shapes = [(27, 32, 64), (3, 48, 5)]
    ws = [_g(rng.standard_normal(s).astype(np.float32)) for s in shapes]
    for single, multi, planes in ((L().btc_weights_to_bf16, L().btc_weights_to_bf16_multi, 1), (L().btc_weights_split3, L().btc_weights_split3_multi, 3)):
        one = [torch.full((2, planes * w.numel()), -1, dtype=torch.int16, device=dev()) for w in ws]
        many = [torch.full((2, planes * w.numel()), -2, dtype=torch.int16, device=dev()) for w in ws]
        for w, s, q in zip(ws, shapes, one):
            check(single(ptr(w), s[0], s[1], s[2], ptr(q[0]), ptr(q[1]), stream_ptr()), "single")
        vp = ctypes.c_void_p * len(ws)
        i32 = ctypes.c_int32 * len(ws)
        check(multi(vp(*[ptr(w) for w in ws]), vp(*[ptr(q[0]) for q in many]), vp(*[ptr(q[1]) for q in many]), i32(*[s[0] for s in shapes]),
                    i32(*[s[1] for s in shapes]), i32(*[s[2] for s in shapes]), len(ws), stream_ptr()), "multi")
        torch.cuda.synchronize()
        for a, b in zip(one, many):
            assert torch.equal(a, b)
