"""Sparse-conv kernels at kernel volumes other than 3 x 3 x 3, at tile edges and at the row counts where the dispatch policy switches.

Every family of csrc/sparse_conv.hip, conv_apply_glds.hip, conv_apply_split.hip, conv_apply_bf16.hip, conv_wgrad.hip, conv_wgrad_x.hip and conv_wgrad_n.hip
takes the number of offsets K at run time: the per-wave offset ballot (64 bits), the compact offset lists, PAIR's odd tail, z-split's item
count, the K-sized map tiles in LDS and the offset groups of the weight-gradient walks all depend on it.  Here each family runs at K from 1
to 512 on synthetic maps (tests/conv_ref.py: exact row counts, rows without neighbours, rows with all K offsets, an offset missing from
whole tiles, offset K - 1 present in the last row of the last partial tile only, maps where every source row has one offset) and on real
rulebooks of the configured kernel shapes.  The bars are the suite's own: bit-exact against the oracle's fmaf chain for the exact kernels,
the float64 bars of tests/test_hip_split.py, tests/test_hip_bf16*.py, tests/test_hip_wgrad_x.py and tests/test_hip_wgrad_n.py for the
others.  Every output buffer starts as NaN, so a row a kernel never stores fails the comparison."""
import contextlib

import numpy as np
import pytest
import torch

from conv_ref import f64_conv, synth_map, wgrad64
from oracle import oracle as orc
from test_hip_core import _rb_both, dev, rand_indices

pytestmark = pytest.mark.gpu

APPLY_KERNEL, APPLY_NT, APPLY_KC, WGRAD_PH, BF16_OPERANDS, WGRAD_PIPE, BN_FUSE, STAGES, SPLIT, SPLIT_Z, LOADERS, WGRAD_X, X_DEPTH, PAIR, NARROW = (
    0, 1, 4, 5, 8, 11, 12, 13, 14, 15, 17, 18, 20, 21, 22)
SMALL_N = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129]


def L():
    from btcdet_amd._lib import lib
    return lib()


@contextlib.contextmanager
def tuned(*pairs):
    try:
        for k, v in pairs:
            assert L().btc_tune_set(k, v) == 0
        yield
    finally:
        for k, _ in pairs:
            L().btc_tune_set(k, 0)


def _g(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dt is None else t.to(dt)


class Case:
    """a layer on a synthetic map: fp32 operands (numpy) and their device copies"""

    def __init__(self, seed, n, K, cin, cout, bf16=False, **map_kw):
        rng = np.random.default_rng(seed)
        self.n, self.K, self.cin, self.cout = n, K, cin, cout
        self.nbr_out, self.nbr_in, self.order = synth_map(rng, n, K, **map_kw)
        self.n_src = self.nbr_in.shape[0]
        rnd = orc.bf16_round if bf16 else (lambda a: a)
        self.feat = rnd(rng.standard_normal((self.n_src, cin)).astype(np.float32))
        self.W = (rng.standard_normal((K, cin, cout)) / np.sqrt(cin * min(K, 8))).astype(np.float32)
        self.bias = rng.standard_normal(cout).astype(np.float32)
        self.dout = rnd(rng.standard_normal((n, cout)).astype(np.float32))
        dt = torch.bfloat16 if bf16 else torch.float32
        self.f, self.d = _g(self.feat, dt), _g(self.dout, dt)
        self.w, self.b = _g(self.W), _g(self.bias)
        self.m_out, self.m_in, self.o = _g(self.nbr_out), _g(self.nbr_in), _g(self.order)

    def apply(self, pass_, operands=0, W=None, order=False, bias=True):
        """btc_conv_apply_src -> result (NaN-poisoned before the launch); pass 0 = forward over nbr_out, 1 = dgrad over nbr_in"""
        from btcdet_amd._lib import check, ptr, stream_ptr
        fwd = pass_ == 0
        src, nbr, rows, cres = (self.f, self.m_out, self.n, self.cout) if fwd else (self.d, self.m_in, self.n_src, self.cin)
        out = torch.full((rows, cres), float("nan"), dtype=src.dtype, device=dev())
        check(L().btc_conv_apply_src(pass_, operands, ptr(src), src.shape[0], ptr(self.w if W is None else W), ptr(self.b) if fwd and bias else None,
                                     ptr(nbr), ptr(self.o) if order else None, rows, self.K, self.cin, self.cout, ptr(out), stream_ptr()),
              "btc_conv_apply_src")
        torch.cuda.synchronize()
        return out

    def oracle(self, pass_, W=None, bias=True):
        W = self.W if W is None else W
        if pass_ == 0:
            return orc.conv_fwd(self.feat, W, self.bias if bias else None, self.nbr_out)
        return orc.conv_dgrad(self.dout, W, self.nbr_in)

    def f64(self, pass_):
        if pass_ == 0:
            return f64_conv(self.feat, self.W, self.nbr_out, False) + self.bias.astype(np.float64)
        return f64_conv(self.dout, self.W, self.nbr_in, True)

    def wgrad(self, feat=None, dout=None):
        from btcdet_amd._lib import check, ptr, stream_ptr
        feat, dout = (self.f if feat is None else feat), (self.d if dout is None else dout)
        fn = L().btc_conv_wgrad_bf16 if feat.dtype == torch.bfloat16 else L().btc_conv_wgrad
        wsb = L().btc_conv_wgrad_ws_bytes(self.n, self.K, self.cin, self.cout, self.n_src)
        ws = torch.empty((max(wsb, 256),), dtype=torch.uint8, device=dev())
        dw = torch.full((self.K, self.cin, self.cout), float("nan"), device=dev())
        check(fn(ptr(feat), ptr(dout), ptr(self.m_out), self.n, ptr(self.m_in), self.n_src, self.K, self.cin, self.cout, ptr(dw), ptr(ws), wsb,
                 stream_ptr()), "btc_conv_wgrad")
        torch.cuda.synchronize()
        return dw

    def wgrad64(self):
        return wgrad64(self.f.float(), self.d.float(), self.m_out, self.K, self.cin, self.cout)


def _exact(c, passes=(0, 1), order=False):
    for p in passes:
        np.testing.assert_array_equal(c.apply(p, order=order).cpu().numpy(), c.oracle(p), err_msg="pass %d" % p)


def _err(a, ref):
    d = a.astype(np.float64) - ref
    return float(np.abs(d).max() / np.abs(ref).max()), float(np.sqrt((d ** 2).mean()) / np.sqrt((ref ** 2).mean()))


def _split_bar(got, exact, ref64, what):
    """tests/test_hip_split.py: at least as close to float64 as the exact chain, within 4e-6 of it, and not its bits"""
    assert not np.array_equal(got, exact), what + ": the exact chain's bits (the split kernel did not run)"
    (mx, rms), (mx_e, rms_e) = _err(got, ref64), _err(exact, ref64)
    assert rms <= 1.1 * rms_e and mx <= 1.5 * mx_e + 2e-7, (what, mx, rms, mx_e, rms_e)
    assert float(np.abs(got - exact).max() / np.abs(exact).max()) <= 4e-6, what


def _wgrad_bar(got, ref, what):
    """tests/test_hip_core.py: every fp32 weight gradient within 1e-4 of the scale of a double-precision reference"""
    assert bool(torch.isfinite(got).all()), what
    assert float((got.double() - ref).abs().max()) <= 1e-4 * (float(ref.abs().max()) + 1e-6), what


def _ensure_scratch():
    """the stream's scratch buffer the z-split launches need (as spconv/ops.py registers it)"""
    from btcdet_amd._lib import check, ptr, stream_ptr
    from btcdet_amd.spconv import ops
    key = (dev().index, stream_ptr())
    if key not in ops._SCRATCH:
        buf = ops._SCRATCH[key] = torch.empty(48 << 20, dtype=torch.uint8, device=dev())
        check(L().btc_set_scratch(stream_ptr(), ptr(buf), buf.numel()), "btc_set_scratch")


# ------------------------------------------------------------------ (a) real rulebooks of the configured kernel shapes
# (kernel, stride, padding, form): subm for odd kernels, strided / plain regular convs, their transposed and inverse forms
RB_KERNELS = [
    ((1, 1, 1), 1, 0, "subm"), ((1, 1, 1), 1, 0, "conv"),
    ((2, 1, 1), (2, 1, 1), 0, "conv"), ((2, 1, 1), (2, 1, 1), 0, "inverse"),
    ((3, 1, 1), (2, 1, 1), 0, "conv"), ((3, 1, 1), (2, 1, 1), 0, "transpose"),
    ((2, 2, 2), 2, 0, "conv"), ((2, 2, 2), 2, 0, "transpose"), ((2, 2, 2), 2, 0, "inverse"),
    ((1, 3, 3), 1, (0, 1, 1), "subm"),
    ((2, 2, 3), (2, 2, 3), 0, "conv"), ((2, 2, 3), (2, 2, 3), 0, "inverse"),
    ((2, 4, 4), 1, 0, "conv"),
    ((3, 11, 1), 1, (1, 5, 0), "subm"),
    ((5, 3, 3), 1, (2, 1, 1), "subm"), ((5, 3, 3), 2, 1, "conv"),
    ((4, 4, 4), 1, 0, "conv"), ((4, 4, 4), 2, 1, "transpose"),
    ((5, 5, 5), 1, 2, "subm"),
]


@pytest.mark.parametrize("k,s,p,form", RB_KERNELS, ids=lambda v: str(v).replace(" ", ""))
def test_rulebooks_and_autograd_at_kernel_volumes(k, s, p, form, exact_conv):
    """ops.build_rulebook == the oracle's rulebook; ops.indice_conv forward and data gradient bit-exact against the oracle, the weight
    gradient within 1e-4 of the scale of float64"""
    from btcdet_amd.spconv import ops
    K = int(np.prod(k))
    rng = np.random.default_rng(K * 7 + len(form))
    shape, B = ((6, 14, 12) if form == "transpose" else (10, 24, 20)), 2
    idx = rand_indices(rng, 900 if form == "transpose" else 2600, B, shape)
    s3, p3 = (s,) * 3 if isinstance(s, int) else s, (p,) * 3 if isinstance(p, int) else p
    (o_idx, o_out, o_in, o_sh), rb = _rb_both(idx, B, shape, k, s3, p3, (1, 1, 1), "conv" if form == "inverse" else form)
    assert rb.nbr_out.shape[1] == K
    assert list(rb.out_shape) == list(o_sh)
    np.testing.assert_array_equal(rb.out_indices.cpu().numpy(), o_idx)
    np.testing.assert_array_equal(rb.nbr_out.cpu().numpy(), o_out)
    np.testing.assert_array_equal(rb.nbr_in.cpu().numpy(), o_in)
    inverse = form == "inverse"
    if inverse:                                        # the inverse conv runs the strided rulebook backwards: result rows = its inputs
        o_out, o_in = o_in, o_out
    n_src, n_res = o_in.shape[0], o_out.shape[0]
    cin, cout = {1: (16, 32), 2: (32, 32), 3: (64, 128), 8: (16, 16), 12: (128, 128)}.get(K, (16, 32) if K <= 64 else (8, 16))
    feat = rng.standard_normal((n_src, cin)).astype(np.float32)
    W = (rng.standard_normal((K, cin, cout)) / np.sqrt(cin * min(K, 8))).astype(np.float32)
    dout = rng.standard_normal((n_res, cout)).astype(np.float32)
    f = _g(feat).requires_grad_(True)
    w = _g(W).requires_grad_(True)
    out = ops.indice_conv(f, w, None, rb, inverse=inverse)
    out.backward(_g(dout))
    ops.join_wgrad()
    np.testing.assert_array_equal(out.detach().cpu().numpy(), orc.conv_fwd(feat, W, None, o_out))
    np.testing.assert_array_equal(f.grad.cpu().numpy(), orc.conv_dgrad(dout, W, o_in))
    _wgrad_bar(w.grad, wgrad64(f.detach(), _g(dout), _g(o_out), K, cin, cout), "wgrad")


# ------------------------------------------------------------------ (b) every kernel family on synthetic maps
K_LE64 = [1, 2, 3, 8, 12, 16, 27, 33, 45, 64]
GLDS_SHAPES = [411, 412, 414, 418, 421, 422, 424, 221, 222, 224, 241, 242, 141, 142]


@pytest.mark.parametrize("shape_code", GLDS_SHAPES)
def test_lds_dma_instances(shape_code):
    """conv_apply_g: every wave shape x reduction chunk 16 / 32 / 64 (keys 0, 1, 4), forward and dgrad bit-exact against the oracle;
    the forward also through a row-order hint"""
    wc, ntw = (shape_code // 10) % 10, shape_code % 10
    cout = 16 * wc * ntw * (2 if wc * ntw <= 2 else 1)
    for j, kc in enumerate((16, 32, 64)):
        i = GLDS_SHAPES.index(shape_code) * 3 + j
        K, n = K_LE64[i % len(K_LE64)], SMALL_N[(i * 3) % len(SMALL_N)]
        c = Case(i, n, K, {64: 64, 32: 96, 16: 48}[kc], cout)
        with tuned((APPLY_KERNEL, 2), (APPLY_NT, shape_code), (APPLY_KC, kc)):
            _exact(c, order=(i % 2 == 1))


# (K, n, cin, cout, nt): Cred % 4 != 0 takes the scalar-load variant (VEC = false) -- forward for cin, dgrad for cout
REG_CASES = [(1, 1, 16, 16, 1), (2, 17, 6, 18, 2), (3, 65, 20, 48, 4), (8, 129, 34, 32, 8), (12, 128, 32, 12, 1), (16, 63, 4, 16, 2),
             (27, 127, 16, 32, 4), (33, 64, 32, 32, 8), (45, 15, 8, 20, 1), (64, 16, 16, 64, 2), (65, 129, 16, 16, 4), (125, 100, 12, 16, 8),
             (216, 65, 16, 8, 2), (343, 130, 8, 16, 8), (512, 129, 16, 16, 8), (512, 1, 4, 4, 1)]


@pytest.mark.parametrize("K,n,cin,cout,nt", REG_CASES)
def test_register_staged_kernel(K, n, cin, cout, nt):
    """conv_apply (key 0 = 1; the only kernel past 64 offsets), every NT, both load variants: bit-exact against the oracle"""
    c = Case(K + n, n, K, cin, cout)
    with tuned((APPLY_KERNEL, 1), (APPLY_NT, nt)):
        _exact(c)


@pytest.mark.parametrize("K,n,cin,cout", [(2, 2047, 4, 16), (2, 2048, 4, 16), (8, 4097, 6, 32), (33, 2048, 4, 16), (64, 2049, 8, 3),
                                          (12, 5000, 32, 3)])
def test_weight_stationary_kernel(K, n, cin, cout):
    """conv_apply_ws (Cred <= 8, Cres <= 32, >= 2048 rows): bit-exact against the oracle, with the register-staged kernel below 2048 rows"""
    _exact(Case(K * 3 + n, n, K, cin, cout, pairs_per_row=4.0))


# conv_apply_s: every case of the S_CASE switch (shape, kc, stages) and the three S_PAIR tiles
S_CASES = [(424, 32, 3), (424, 32, 4), (424, 64, 2), (224, 32, 3), (224, 64, 2), (224, 32, 4), (222, 64, 2), (222, 32, 3), (222, 32, 4),
           (422, 64, 3), (422, 32, 3), (422, 32, 4), (422, 64, 2), (412, 64, 2), (412, 32, 3), (412, 32, 4), (812, 64, 2), (812, 32, 3),
           (812, 32, 4), (414, 64, 2), (414, 32, 3), (814, 64, 2), (814, 32, 3), (418, 64, 2), (418, 32, 3), (818, 32, 3),
           (412, "pair", 2), (812, "pair", 2), (422, "pair", 2)]
S_K = [3, 8, 12, 16, 27, 33, 64, 1, 2, 45]


def _split_planes(c):
    from btcdet_amd._lib import check, ptr, stream_ptr
    q = torch.empty((2, 3 * c.w.numel()), dtype=torch.bfloat16, device=dev())
    check(L().btc_weights_split3(ptr(c.w), c.K, c.cin, c.cout, ptr(q[0]), ptr(q[1]), stream_ptr()), "btc_weights_split3")
    return q


@pytest.mark.parametrize("shape,kc,stages", S_CASES, ids=lambda v: str(v))
def test_split_kernel_instances(shape, kc, stages):
    """conv_apply_s forced to each instance (keys 1, 4, 13, 15 = 1, 21): the float64 bar of test_split_kernel_vs_fp64_and_exact_chain.
    Loader waves (key 17) and, on the 32-channel tiles, one or two offsets per item (key 21) give the same bits"""
    _ensure_scratch()
    i = S_CASES.index((shape, kc, stages))
    K, n = S_K[i % len(S_K)], [65, 129, 127, 1000, 2500, 4999][i % 6]
    tn = 16 * ((shape // 10) % 10) * (shape % 10)
    pair = kc == "pair"
    cin = 32 if pair else (64 if kc == 64 else 96)
    c = Case(100 + i, n, K, cin, tn, pairs_per_row=6.0)
    q = _split_planes(c)
    keys = [(APPLY_NT, shape), (SPLIT_Z, 1), (PAIR, 2 if pair else 1)]
    if not pair:
        keys += [(APPLY_KC, kc), (STAGES, stages if kc == 32 or shape == 422 else 0)]
    with tuned(*keys):
        got = c.apply(0, 3, W=q[1])
    _split_bar(got.cpu().numpy(), c.oracle(0), c.f64(0), "shape %s kc %s" % (shape, kc))
    for lw in (1, 2, 4):
        with tuned(*keys, (LOADERS, lw)):
            assert torch.equal(c.apply(0, 3, W=q[1]), got), "loaders %d" % lw
    if pair:
        with tuned(*[kv for kv in keys if kv[0] != PAIR], (PAIR, 1)):
            alt = c.apply(0, 3, W=q[1])
        assert torch.equal(alt, got), "PAIR"


@pytest.mark.parametrize("K,cin,cout,n", [(12, 128, 128, 3000), (16, 64, 64, 3500), (33, 64, 128, 2000), (27, 96, 64, 999), (64, 64, 64, 129)])
def test_split_kernel_z_split(K, cin, cout, n):
    """z-split (key 15 = 2..4 workgroups per tile, items = K Cred / kc >= 12): forward and dgrad through the mirror-free maps, each Z
    within the float64 bar; the dgrad through the stream's scratch and split_reduce"""
    _ensure_scratch()
    c = Case(K + cin + n, n, K, cin, cout, pairs_per_row=6.0)
    q = _split_planes(c)
    ex, ref = (c.oracle(0), c.oracle(1)), (c.f64(0), c.f64(1))
    runs = {}
    for z in (1, 2, 3, 4):
        with tuned((SPLIT_Z, z)):
            runs[z] = [c.apply(p, 3, W=q[1 - p]).cpu().numpy() for p in (0, 1)]
        for p in (0, 1):
            _split_bar(runs[z][p], ex[p], ref[p], "Z %d pass %d" % (z, p))
    assert not all(np.array_equal(runs[1][p], runs[4][p]) for p in (0, 1)), "z-split never ran"


# (K, n, cin, cout, pair key): conv_apply_b -- bf16 activations and bf16 weights
B_CASES = [(1, 17, 32, 16, 0), (3, 129, 64, 64, 0), (8, 5000, 32, 32, 0), (12, 64, 128, 128, 0), (16, 6000, 32, 64, 0), (27, 127, 64, 48, 0),
           (33, 65, 32, 32, 2), (45, 1, 64, 16, 0), (64, 5001, 32, 32, 0), (64, 128, 96, 64, 0)]


def _bf16_check(got, ref, what):
    """tests/test_hip_bf16_mfma.py: |out - ref| <= 2^-8 |ref| + 2e-6 scale against the fmaf chain over the same bf16 operands"""
    err, bound = np.abs(got - ref), 2.0 ** -8 * np.abs(ref) + 2e-6 * float(np.abs(ref).max())
    assert float((err / bound).max()) <= 1.0, what


@pytest.mark.parametrize("K,n,cin,cout,pair", B_CASES)
def test_bf16_operand_kernel(K, n, cin, cout, pair):
    """conv_apply_b (BTC_OPERANDS_BF16): the bar of test_hip_bf16_mfma.py in both passes where the reduction allows it, not the bits of the
    fp32-weight chain; one or two offsets per item (key 21) give the same bits"""
    from btcdet_amd._lib import check, ptr, stream_ptr
    c = Case(K * 5 + n, n, K, cin, cout, bf16=True, pairs_per_row=6.0)
    q = torch.empty((2, c.w.numel()), dtype=torch.bfloat16, device=dev())
    check(L().btc_weights_to_bf16(ptr(c.w), K, cin, cout, ptr(q[0]), ptr(q[1]), stream_ptr()), "btc_weights_to_bf16")
    Wq = orc.bf16_round(c.W)
    for p in (0, 1):
        if L().btc_conv_bf16w_supported(K, cin if p == 0 else cout, cout if p == 0 else cin) != 1:
            continue
        with tuned((PAIR, pair)):
            got = c.apply(p, 2, W=q[1 - p]).float().cpu().numpy()
        _bf16_check(got, c.oracle(p, W=Wq), "pass %d" % p)
        assert not np.array_equal(got, orc.bf16_round(c.oracle(p))), "the fp32-weight chain's bits (the bf16-operand kernel did not run)"
        if (cin if p == 0 else cout) == 32:
            with tuned((PAIR, 1 if pair == 2 else 2)):
                assert np.array_equal(c.apply(p, 2, W=q[1 - p]).float().cpu().numpy(), got), "PAIR"


@pytest.mark.parametrize("K,n", [(2, 1), (3, 129), (12, 8191), (12, 8192), (33, 64), (64, 65)])
def test_bf16_activations_fp32_weights(K, n):
    """BTC_OPERANDS_BF16_ACT (what key 8 = 1 selects in the bindings): conv_apply_g's fmaf chain over bf16 activations -- the oracle's
    result rounded to bf16, bit for bit (tests/test_hip_bf16.py)"""
    c = Case(K + n, n, K, 64, 64, bf16=True, pairs_per_row=5.0)
    for p in (0, 1):
        got = c.apply(p, 1).float().cpu().numpy()
        np.testing.assert_array_equal(got, orc.bf16_round(c.oracle(p)), err_msg="pass %d" % p)


@pytest.mark.parametrize("k,pad", [((1, 1, 1), 0), ((1, 3, 3), (0, 1, 1)), ((3, 3, 3), 1), ((5, 3, 3), (2, 1, 1)), ((5, 5, 5), 2)])
def test_mirrored_dgrad_equals_the_explicit_map(k, pad):
    """BTC_PASS_DGRAD_MIRROR on a submanifold rulebook's forward map == BTC_PASS_DGRAD on its materialised backward map, bit for bit, in
    every family that takes the layer (fp32 policy, register-staged, LDS-DMA, weight-stationary, split operands, bf16 operands)"""
    from btcdet_amd._lib import check, ptr, stream_ptr
    from btcdet_amd.spconv import ops
    K = int(np.prod(k))
    rng = np.random.default_rng(K)
    shape, B = (10, 24, 20), 2
    idx = rand_indices(rng, 2600, B, shape)
    p3 = (pad,) * 3 if isinstance(pad, int) else pad
    rb = ops.build_rulebook(_g(idx), B, shape, k, 1, p3, 1, 0, True, False)
    n = rb.nbr_out.shape[0]
    assert rb.mirrored and n >= 2048
    nbr_in = rb.nbr_in.contiguous()
    _ensure_scratch()

    def both(cin, cout, operands, W, keys=()):
        src = torch.from_numpy(rng.standard_normal((n, cout)).astype(np.float32)).to(dev())
        if operands == 2:
            src = src.to(torch.bfloat16)
        outs = []
        for pass_, m in ((1, nbr_in), (2, rb.nbr_out)):
            out = torch.full((n, cin), float("nan"), dtype=src.dtype, device=dev())
            with tuned(*keys):
                check(L().btc_conv_apply_src(pass_, operands, ptr(src), n, ptr(W), None, ptr(m), None, n, K, cin, cout, ptr(out), stream_ptr()),
                      "dgrad")
            outs.append(out)
        assert not bool(outs[0].isnan().any())
        assert torch.equal(outs[0], outs[1]), (cin, cout, operands, keys)

    for cin, cout, keys in ((32, 64, ()), (16, 16, ((APPLY_KERNEL, 1),)), (48, 6, ((APPLY_KERNEL, 1), (APPLY_NT, 2))), (16, 4, ()),
                            (64, 32, ((APPLY_KERNEL, 2),)), (32, 16, ((APPLY_KERNEL, 2), (APPLY_NT, 141)))):
        if K > 64 and keys and keys[0] == (APPLY_KERNEL, 2):
            continue
        both(cin, cout, 0, torch.from_numpy((rng.standard_normal((K, cin, cout)) / 8).astype(np.float32)).to(dev()), keys)
    if K <= 64:
        w = torch.from_numpy((rng.standard_normal((K, 64, 64)) / 8).astype(np.float32)).to(dev())
        q = torch.empty((2, 3 * w.numel()), dtype=torch.bfloat16, device=dev())
        check(L().btc_weights_split3(ptr(w), K, 64, 64, ptr(q[0]), ptr(q[1]), stream_ptr()), "split3")
        both(64, 64, 3, q[0])
        qb = torch.empty((2, w.numel()), dtype=torch.bfloat16, device=dev())
        check(L().btc_weights_to_bf16(ptr(w), K, 64, 64, ptr(qb[0]), ptr(qb[1]), stream_ptr()), "to_bf16")
        both(64, 64, 2, qb[0])


@pytest.mark.parametrize("K,cin,cout,n", [(3, 16, 16, 3000), (12, 4, 16, 6000), (12, 128, 128, 3000), (33, 64, 128, 900), (64, 32, 32, 129),
                                          (125, 20, 48, 700), (8, 34, 32, 5000)])
def test_fused_batch_statistics(K, cin, cout, n):
    """btc_conv_bn_relu_fwd with the statistics in the conv epilogue (or in split_reduce, 128 -> 128 at 3 K rows: z-split) against the
    separate statistics pass (key 12 = 1): the bar of test_conv_epilogue_batch_statistics_match_the_separate_pass"""
    from btcdet_amd.spconv import fused_bn
    _ensure_scratch()
    c = Case(K * 11 + n, n, K, cin, cout, pairs_per_row=6.0)
    rng = np.random.default_rng(n)
    gamma, beta = _g(rng.uniform(0.5, 1.5, cout).astype(np.float32)), _g(rng.uniform(-0.3, 0.3, cout).astype(np.float32))
    outs = []
    for tune in (0, 1, 0):
        rm, rv = torch.zeros(cout, device=dev()), torch.ones(cout, device=dev())
        nbt = torch.zeros((), dtype=torch.long, device=dev())
        with tuned((BN_FUSE, tune)):
            x, y, stats = fused_bn.conv_bn_forward(c.f, c.w, None, c.m_out, None, gamma, beta, rm, rv, nbt, 0.01, 1e-3, True)
            torch.cuda.synchronize()
        outs.append((x, y, stats, rm, rv, int(nbt)))
    assert torch.equal(outs[0][0], outs[1][0])
    if L().btc_conv_split_wanted(K, cin, cout, n) != 1:
        np.testing.assert_array_equal(outs[0][0].cpu().numpy(), c.oracle(0, bias=False))
    assert bool((fused_bn.fuse_ws(dev()) == 0).all())
    for a, b in ((outs[0], outs[1]), (outs[0], outs[2])):
        assert a[5] == b[5] == 1
        np.testing.assert_allclose(a[2].cpu().numpy(), b[2].cpu().numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(a[3].cpu().numpy(), b[3].cpu().numpy(), rtol=2e-6, atol=1e-8)
        np.testing.assert_allclose(a[4].cpu().numpy(), b[4].cpu().numpy(), rtol=2e-6, atol=1e-8)
        np.testing.assert_allclose(a[1].cpu().numpy(), b[1].cpu().numpy(), rtol=1e-5, atol=1e-5)
    ref = torch.nn.functional.batch_norm(outs[0][0], None, None, gamma, beta, True, 0.0, 1e-3).relu()
    np.testing.assert_allclose(outs[0][1].cpu().numpy(), ref.cpu().numpy(), rtol=2e-5, atol=2e-5)


# ------------------------------------------------------------------ weight gradient
# conv_wgrad_rows_p: (cin, cout) -> offsets per group KB x PH (full PH; key 5 also asks for PH / 2): K = a multiple of it, a tail of 1,
# a single partial group
ROWS_P = [(16, 16, 16, 3), (16, 16, 17, 5000), (16, 16, 32, 4096), (32, 32, 33, 4500), (32, 32, 64, 4096), (32, 32, 12, 6000),
          (64, 64, 12, 4096), (64, 64, 33, 4200), (32, 64, 17, 5000), (64, 32, 64, 4100)]


@pytest.mark.parametrize("cin,cout,K,n", ROWS_P)
def test_wgrad_rows_pipelined_every_phase_count(cin, cout, K, n):
    full_ph = {(16, 16): 4, (32, 32): 8, (64, 64): 4, (32, 64): 4, (64, 32): 8}[(cin, cout)]
    n = max(n, 4096)
    c = Case(cin + K + n, n, K, cin, cout, pairs_per_row=4.0)
    ref = c.wgrad64()
    for ph in (full_ph, full_ph // 2):
        with tuned((WGRAD_X, 1), (NARROW, 1), (WGRAD_PH, ph)):
            _wgrad_bar(c.wgrad(), ref, "PH %d" % ph)


@pytest.mark.parametrize("K", [3, 12, 29, 33, 64])
def test_wgrad_two_barrier_kernel_every_phase_count(K):
    """conv_wgrad_rows (key 11 = 1), 32 -> 32: four offsets per phase, PH = 1, 2, 4, 7 (key 5)"""
    c = Case(K, 4500, K, 32, 32, pairs_per_row=4.0)
    ref = c.wgrad64()
    for ph in (1, 2, 4, 7):
        with tuned((WGRAD_X, 1), (NARROW, 1), (WGRAD_PIPE, 1), (WGRAD_PH, ph)):
            _wgrad_bar(c.wgrad(), ref, "PH %d" % ph)


@pytest.mark.parametrize("K,n,cin,cout", [(65, 4096, 32, 32), (125, 3000, 16, 16), (12, 4095, 32, 32), (33, 129, 20, 48), (512, 700, 8, 16),
                                          (216, 1, 16, 16), (1, 64, 16, 16)])
def test_wgrad_offset_major_kernels(K, n, cin, cout):
    """conv_wgrad_partial_p / conv_wgrad_partial (key 11 = 1): past 64 offsets, under 4096 rows, and channel counts without a row tile"""
    c = Case(K + n, n, K, cin, cout, pairs_per_row=4.0)
    ref = c.wgrad64()
    for pipe in (0, 1):
        with tuned((WGRAD_X, 1), (NARROW, 1), (WGRAD_PIPE, pipe)):
            _wgrad_bar(c.wgrad(), ref, "pipe key %d" % pipe)


@pytest.mark.parametrize("K,n,cin,cout", [(3, 2048, 64, 128), (12, 4096, 128, 128), (16, 3000, 32, 32), (33, 2500, 32, 64), (64, 2049, 32, 32),
                                          (8, 6000, 64, 5)])
def test_wgrad_bf16_pipe_both_modes(K, n, cin, cout):
    """conv_wgrad_x (key 18): fp32 activations (mode 1) within the bars of test_hip_wgrad_x.py against the fp32 chain and float64, bf16
    activations (mode 0) within 4e-6 of the scale of float64 over the same bf16 inputs; items in flight (key 20) change no bit"""
    c = Case(K * 13 + n, n, K, cin, cout, pairs_per_row=5.0)
    ref = c.wgrad64()
    scale = float(ref.abs().max()) + 1e-12
    with tuned((NARROW, 1)):
        got = c.wgrad()
        for depth in (1, 2):
            with tuned((X_DEPTH, depth)):
                assert torch.equal(c.wgrad(), got), "depth %d" % depth
        with tuned((WGRAD_X, 1)):
            old = c.wgrad()
    assert not torch.equal(got, old), "the bf16-pipe kernel was not taken"
    e_new, e_old = float((got.double() - ref).abs().max()) / scale, float((old.double() - ref).abs().max()) / scale
    r_new, r_old = float((got.double() - ref).pow(2).mean().sqrt()) / scale, float((old.double() - ref).pow(2).mean().sqrt()) / scale
    assert e_new <= 1e-4
    assert e_new <= 1.5 * e_old + 2e-7 and r_new <= 1.5 * r_old + 5e-8, (e_new, e_old, r_new, r_old)
    fb, db = c.f.to(torch.bfloat16), c.d.to(torch.bfloat16)
    ref_b = wgrad64(fb.float(), db.float(), c.m_out, K, cin, cout)
    with tuned((NARROW, 1)):
        got_b = c.wgrad(fb, db)
        with tuned((WGRAD_X, 1)):
            assert not torch.equal(got_b, c.wgrad(fb, db)), "the bf16-pipe kernel was not taken (bf16)"
    assert float((got_b.double() - ref_b).abs().max()) <= 4e-6 * (float(ref_b.abs().max()) + 1e-12)


@pytest.mark.parametrize("K,n,cin,cout", [(8, 2048, 32, 8), (12, 3000, 32, 5), (33, 5000, 16, 5), (64, 2500, 64, 2), (3, 9000, 48, 3),
                                          (27, 2047, 32, 5)])
def test_wgrad_narrow_result_kernel(K, n, cin, cout):
    """conv_wgrad_n (key 22): the bars of test_hip_wgrad_n.py against the fp32 chain and float64 -- and below 2048 input rows the kernels of
    before, bit for bit"""
    c = Case(K * 17 + n, n, K, cin, cout, pairs_per_row=5.0)
    ref = c.wgrad64()
    scale = float(ref.abs().max()) + 1e-12
    got = c.wgrad()
    with tuned((NARROW, 1), (WGRAD_X, 1)):
        old = c.wgrad()
    if c.n_src < 2048:
        with tuned((NARROW, 1)):
            assert torch.equal(got, c.wgrad())
        _wgrad_bar(got, ref, "below 2048 rows")
        return
    assert not torch.equal(got, old), "the narrow kernel was not taken"
    e_new, e_old = float((got.double() - ref).abs().max()) / scale, float((old.double() - ref).abs().max()) / scale
    r_new, r_old = float((got.double() - ref).pow(2).mean().sqrt()) / scale, float((old.double() - ref).pow(2).mean().sqrt()) / scale
    assert e_new <= 1e-4
    assert e_new <= max(1.5 * e_old + 2e-7, 1e-6) and r_new <= max(1.5 * r_old + 5e-8, 2e-7), (e_new, e_old, r_new, r_old)


# ------------------------------------------------------------------ the built-in policy on both sides of its row-count thresholds
# (K, cin, cout, n, exact): n - 1 and n; `exact` = key 14 = 1 (the exact kernels only), else the bindings' own choice
POLICY = [(8, 4, 16, 2048, False), (33, 16, 16, 2048, False), (12, 128, 128, 2500, False), (33, 64, 64, 4000, False), (12, 20, 32, 4096, False),
          (12, 64, 64, 5000, False), (8, 32, 64, 6000, False), (3, 128, 128, 7000, True), (12, 128, 128, 10000, False), (12, 64, 64, 11000, True),
          (8, 32, 64, 13000, True), (3, 128, 128, 16385, True), (3, 128, 128, 19500, True), (12, 32, 32, 20000, False), (12, 64, 64, 22000, False),
          (3, 32, 32, 100000, True), (3, 32, 32, 100000, False)]


@pytest.mark.parametrize("K,cin,cout,n,exact", POLICY)
def test_policy_thresholds(K, cin, cout, n, exact):
    """ops' autograd function through the compiled binding, one row below a threshold and at it: forward and dgrad bit-exact against the
    oracle where the exact kernels take them, within the split kernel's float64 bar where btc_conv_split_wanted says it does; the weight
    gradient within 1e-4 of the scale of float64"""
    from btcdet_amd.spconv import ops
    for rows in (n - 1, n):
        c = Case(K + cin + rows, rows, K, cin, cout, pairs_per_row=3.0)
        with tuned((SPLIT, 1 if exact else 0)):
            f = c.f.clone().requires_grad_(True)
            w = c.w.clone().requires_grad_(True)
            y = ops.SparseConvFunction.apply(f, w, c.b, c.m_out, c.m_in)
            y.backward(c.d)
            ops.join_wgrad()
            torch.cuda.synchronize()
            split = (L().btc_conv_split_wanted(K, cin, cout, rows) == 1, L().btc_conv_split_wanted(K, cout, cin, c.n_src) == 1)
        for p, got in ((0, y.detach()), (1, f.grad)):
            got = got.cpu().numpy()
            if split[p]:
                _split_bar(got, c.oracle(p), c.f64(p), "%d rows pass %d" % (rows, p))
            else:
                np.testing.assert_array_equal(got, c.oracle(p), err_msg="%d rows pass %d" % (rows, p))
        _wgrad_bar(w.grad.view(K, cin, cout), c.wgrad64(), "%d rows" % rows)


# ------------------------------------------------------------------ the K limit
def test_k_limit_is_refused_on_the_host():
    """BTC_CONV_K_MAX = 512 offsets: K = 512 runs (test_register_staged_kernel, test_wgrad_offset_major_kernels), K = 513 is refused with
    BTC_EINVAL and a message naming the limit -- by btc_conv_apply_src, btc_conv_wgrad, btc_conv_bn_relu_fwd and the compiled binding"""
    from btcdet_amd._lib import BtcHipError, ptr, stream_ptr
    from btcdet_amd.spconv import fused_bn, ops
    c = Case(3, 70, 513, 16, 16, pairs_per_row=4.0)
    out = torch.zeros((c.n, c.cout), device=dev())
    for pass_ in (0, 1, 2):
        rc = L().btc_conv_apply_src(pass_, 0, ptr(c.f), c.n_src, ptr(c.w), None, ptr(c.m_out), None, c.n, c.K, c.cin, c.cout, ptr(out), stream_ptr())
        assert rc == -1 and b"BTC_CONV_K_MAX = 512" in L().btc_last_error()
    ws = torch.empty((1 << 20,), dtype=torch.uint8, device=dev())
    dw = torch.zeros((c.K, c.cin, c.cout), device=dev())
    rc = L().btc_conv_wgrad(ptr(c.f), ptr(c.d), ptr(c.m_out), c.n, ptr(c.m_in), c.n_src, c.K, c.cin, c.cout, ptr(dw), ptr(ws), ws.numel(), stream_ptr())
    assert rc == -1 and b"BTC_CONV_K_MAX = 512" in L().btc_last_error()
    with pytest.raises((BtcHipError, RuntimeError), match="BTC_CONV_K_MAX = 512"):     # (the compiled binding raises RuntimeError)
        ops.SparseConvFunction.apply(c.f, c.w, None, c.m_out, c.m_in)
    g, b = torch.ones(c.cout, device=dev()), torch.zeros(c.cout, device=dev())
    with pytest.raises(BtcHipError, match="BTC_CONV_K_MAX = 512"):
        fused_bn.conv_bn_forward(c.f, c.w, None, c.m_out, None, g, b, torch.zeros(c.cout, device=dev()), torch.ones(c.cout, device=dev()),
                                 torch.zeros((), dtype=torch.long, device=dev()), 0.01, 1e-3, True)
    assert bool((out == 0).all()) and bool((dw == 0).all())
    c = Case(4, 70, 512, 16, 16, pairs_per_row=4.0)
    _exact(c)
    _wgrad_bar(c.wgrad(), c.wgrad64(), "K = 512")


def test_stride_equals_kernel_maps():
    """every source row in exactly one pair (the (2,2,3) stride-(2,2,3) ROI layer, K = 12; the (2,1,1) stride-2 layer, K = 2): the exact
    kernels bit-exact in both passes, the split kernel within its bar, the weight gradient within 1e-4 of the scale"""
    _ensure_scratch()
    for K, n, cin, cout in ((12, 3000, 128, 128), (2, 4097, 64, 64), (12, 129, 32, 32)):
        c = Case(K + n, n, K, cin, cout, one_per_source=True, pairs_per_row=4.0)
        with tuned((APPLY_KERNEL, 2)):
            _exact(c)
        with tuned((APPLY_KERNEL, 1)):
            _exact(c)
        q = _split_planes(c)
        _split_bar(c.apply(0, 3, W=q[1]).cpu().numpy(), c.oracle(0), c.f64(0), "split fwd")
        _split_bar(c.apply(1, 3, W=q[0]).cpu().numpy(), c.oracle(1), c.f64(1), "split dgrad")
        _wgrad_bar(c.wgrad(), c.wgrad64(), "wgrad")
