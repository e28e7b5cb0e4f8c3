"""Eval-mode conv -> BatchNorm(running statistics) -> ReLU in one launch (btc_conv_bn_eval_fwd, include/btcdet_hip_infer.h; tuning key 23).

The acceptance condition is BIT IDENTITY with the three launches it replaces -- btc_conv_apply_src, then btc_bn_relu_fwd(training = 0)
(bn_eval_stats + bn_apply) -- in every operand mode and kernel family, over the case tables of tests/test_hip_conv_kernel_volumes.py.
On the exact kernels the result is also held to the oracle's conv followed by the eval BatchNorm in numpy at rtol = atol = 1e-5 (the
bound tests/test_hip_roi_microscenes.py holds that composition to).  Then the routing of both bindings, and the whole eval forward."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from test_hip_core import dev, rand_indices
from test_hip_conv_kernel_volumes import (APPLY_KC, APPLY_KERNEL, APPLY_NT, B_CASES, BF16_OPERANDS, GLDS_SHAPES, K_LE64, LOADERS, PAIR, REG_CASES,
                                          S_CASES, S_K, SMALL_N, SPLIT, SPLIT_Z, STAGES, Case, L, _ensure_scratch, _g, _split_planes, tuned)

pytestmark = pytest.mark.gpu

EVAL_FOLD = 23
EPS = 1e-3
# (bias, relu, affine, row-order hint)
VARIANTS = [(True, True, True, False), (False, False, True, True), (True, True, False, True), (False, True, True, False), (True, False, False, False)]


class Bn:
    """eval-mode BatchNorm constants of a layer with C result channels"""

    def __init__(self, seed, C):
        rng = np.random.default_rng(seed)
        self.gamma, self.beta = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.uniform(-0.5, 0.5, C).astype(np.float32)
        self.mean, self.var = rng.uniform(-0.3, 0.3, C).astype(np.float32), rng.uniform(0.3, 1.7, C).astype(np.float32)
        self.g, self.b, self.rm, self.rv = _g(self.gamma), _g(self.beta), _g(self.mean), _g(self.var)
        self.rm0, self.rv0 = self.rm.clone(), self.rv.clone()

    def untouched(self):
        return torch.equal(self.rm, self.rm0) and torch.equal(self.rv, self.rv0)


def unfused(c, bn, operands, W, bias, relu, affine, order):
    """today's path: btc_conv_apply_src -> btc_bn_relu_fwd[_bf16](training = 0)"""
    from btcdet_amd._lib import check, ptr, stream_ptr
    x = c.apply(0, operands, W=W, order=order, bias=bias)
    y = torch.full_like(x, float("nan"))
    C = c.cout
    stats = torch.empty((2, C), device=dev())
    need = L().btc_bn_ws_bytes(C)
    ws = torch.zeros((need,), dtype=torch.uint8, device=dev())
    fn = L().btc_bn_relu_fwd_bf16 if x.dtype == torch.bfloat16 else L().btc_bn_relu_fwd
    check(fn(ptr(x), c.n, C, ptr(bn.g) if affine else None, ptr(bn.b) if affine else None, ptr(bn.rm), ptr(bn.rv), None, 0.01, EPS, 0, int(relu),
             ptr(y), ptr(stats[0]), ptr(stats[1]), ptr(ws), need, stream_ptr()), "btc_bn_relu_fwd")
    torch.cuda.synchronize()
    return x, y


def folded(c, bn, operands, W, bias, relu, affine, order):
    from btcdet_amd._lib import check, ptr, stream_ptr
    y = torch.full((c.n, c.cout), float("nan"), dtype=c.f.dtype, device=dev())
    check(L().btc_conv_bn_eval_fwd(operands, ptr(c.f), c.f.shape[0], ptr(c.w if W is None else W), ptr(c.b) if bias else None, ptr(c.m_out),
                                   ptr(c.o) if order else None, c.n, c.K, c.cin, c.cout, ptr(bn.g) if affine else None, ptr(bn.b) if affine else None,
                                   ptr(bn.rm), ptr(bn.rv), EPS, int(relu), ptr(y), stream_ptr()), "btc_conv_bn_eval_fwd")
    torch.cuda.synchronize()
    return y


def same_bits(c, operands=0, W=None, variants=VARIANTS, oracle=False, what=""):
    bn = Bn(c.n + c.K, c.cout)
    for bias, relu, affine, order in variants:
        tag = "%s bias=%d relu=%d affine=%d order=%d" % (what, bias, relu, affine, order)
        x, ref = unfused(c, bn, operands, W, bias, relu, affine, order)
        got = folded(c, bn, operands, W, bias, relu, affine, order)
        assert not bool(ref.isnan().any()) and not bool(got.isnan().any()), tag
        assert torch.equal(got, ref), tag + ": %d of %d elements differ" % (int((got != ref).sum()), got.numel())
        assert torch.equal(folded(c, bn, operands, W, bias, relu, affine, order), got), tag + ": run to run"
        assert bn.untouched(), tag + ": running statistics written"
        if oracle:
            xr = orc.conv_fwd(c.feat, c.W, c.bias if bias else None, c.nbr_out)
            np.testing.assert_array_equal(x.cpu().numpy(), xr, err_msg=tag)     # (the exact kernel did run)
            g, b = (bn.gamma, bn.beta) if affine else (np.float32(1), np.float32(0))
            yr = (xr - bn.mean) / np.sqrt(bn.var + EPS) * g + b
            yr = (np.maximum(yr, 0) if relu else yr).astype(np.float32)
            np.testing.assert_allclose(got.cpu().numpy(), yr, rtol=1e-5, atol=1e-5, err_msg=tag)
        if relu:
            assert float(got.float().min()) >= 0.0


# ------------------------------------------------------------------ BTC_OPERANDS_F32: the two exact kernels and the narrow instances
@pytest.mark.parametrize("K,n,cin,cout,nt", REG_CASES)
def test_register_staged_kernel(K, n, cin, cout, nt):
    """conv_apply (key 0 = 1), every NT, both load variants, K up to 512: fold = unfused bit for bit, and the oracle composition"""
    c = Case(K + n, n, K, cin, cout)
    with tuned((APPLY_KERNEL, 1), (APPLY_NT, nt)):
        same_bits(c, oracle=True, what="conv_apply nt %d" % nt)


@pytest.mark.parametrize("shape_code", GLDS_SHAPES)
def test_lds_dma_instances(shape_code):
    """conv_apply_g (key 0 = 2): every wave shape x reduction chunk of tests/test_hip_conv_kernel_volumes.py::test_lds_dma_instances"""
    wc, ntw = (shape_code // 10) % 10, shape_code % 10
    cout = 16 * wc * ntw * (2 if wc * ntw <= 2 else 1)
    for j, kc in enumerate((16, 32, 64)):
        i = GLDS_SHAPES.index(shape_code) * 3 + j
        K, n = K_LE64[i % len(K_LE64)], SMALL_N[(i * 3) % len(SMALL_N)]
        c = Case(i, n, K, {64: 64, 32: 96, 16: 48}[kc], cout)
        with tuned((APPLY_KERNEL, 2), (APPLY_NT, shape_code), (APPLY_KC, kc)):
            same_bits(c, variants=VARIANTS[j:j + 3], oracle=True, what="conv_apply_g %d kc %d" % (shape_code, kc))


@pytest.mark.parametrize("K,n,cin,cout", [(2, 2047, 4, 16), (2, 2048, 4, 16), (8, 4097, 6, 32), (33, 2048, 4, 16), (64, 2049, 8, 3), (12, 5000, 8, 20)])
def test_weight_stationary_kernel(K, n, cin, cout):
    """conv_apply_ws (Cred <= 8, Cres <= 32, >= 2048 rows; the fold has instances of its own there) and the policy's choice around it"""
    same_bits(Case(K * 3 + n, n, K, cin, cout, pairs_per_row=4.0), oracle=True, what="conv_apply_ws")


@pytest.mark.parametrize("n", SMALL_N + [2500, 8191])
def test_policy_choice_at_tile_edges(n):
    """no key set: whatever the built-in policy launches for a 27-offset 32 -> 64 layer at the row counts around the tile sizes"""
    same_bits(Case(n, n, 27, 32, 64, pairs_per_row=5.0), variants=VARIANTS[:3], oracle=True, what="policy n %d" % n)


# ------------------------------------------------------------------ BTC_OPERANDS_F32_SPLIT
@pytest.mark.parametrize("shape,kc,stages", S_CASES, ids=lambda v: str(v))
def test_split_kernel_instances(shape, kc, stages):
    """conv_apply_s forced to each instance as tests/test_hip_conv_kernel_volumes.py::test_split_kernel_instances does (key 15 = 1: the
    epilogue is the conv kernel's); loader waves (key 17) and one / two offsets per item (key 21 = 1, 2) give the same bits"""
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
    v = VARIANTS[i % 3:i % 3 + 2]
    with tuned(*keys):
        same_bits(c, 3, q[1], variants=v, what="conv_apply_s %s %s" % (shape, kc))
        bn = Bn(c.n + c.K, c.cout)
        got = folded(c, bn, 3, q[1], *v[0])
        assert not torch.equal(unfused(c, bn, 3, q[1], *v[0])[0], torch.from_numpy(c.oracle(0, bias=v[0][0])).to(dev())), "the split kernel did not run"
    for lw in (2, 4):
        with tuned(*keys, (LOADERS, lw)):
            assert torch.equal(folded(c, bn, 3, q[1], *v[0]), got), "loaders %d" % lw
    if pair:
        with tuned(*[kv for kv in keys if kv[0] != PAIR], (PAIR, 1)):
            assert torch.equal(folded(c, bn, 3, q[1], *v[0]), got), "PAIR"


@pytest.mark.parametrize("K,cin,cout,n", [(12, 128, 128, 3000), (16, 64, 64, 3500), (33, 64, 128, 2000), (27, 96, 64, 999), (64, 64, 64, 129)])
def test_split_kernel_z_split(K, cin, cout, n):
    """z-split (key 15 = 2..4): the affine and the ReLU move into split_reduce; fold = unfused at every Z, and the built-in choice"""
    _ensure_scratch()
    c = Case(K + cin + n, n, K, cin, cout, pairs_per_row=6.0)
    q = _split_planes(c)
    for z in (0, 1, 2, 3, 4):
        with tuned((SPLIT_Z, z)):
            same_bits(c, 3, q[1], variants=VARIANTS[z % 3:z % 3 + 2], what="Z %d" % z)


# ------------------------------------------------------------------ bf16 activations
@pytest.mark.parametrize("K,n,cout", [(2, 1, 64), (3, 129, 64), (12, 8191, 64), (12, 8192, 64), (33, 64, 128), (64, 65, 32), (27, 127, 16), (8, 17, 48)])
def test_bf16_activations_fp32_weights(K, n, cout):
    """BTC_OPERANDS_BF16_ACT (what key 8 = 1 selects in the bindings): every bf16 instance of conv_apply_g; the transform reads the
    conv result rounded to bf16, as bn_apply does"""
    c = Case(K + n, n, K, 64, cout, bf16=True, pairs_per_row=5.0)
    same_bits(c, 1, what="bf16 activations")
    # ... and that rounding is real: the fp32 transform of the unrounded chain differs somewhere
    bn = Bn(c.n + c.K, c.cout)
    xr = orc.bf16_round(orc.conv_fwd(c.feat, c.W, c.bias, c.nbr_out))
    yr = orc.bf16_round(np.maximum((xr - bn.mean) / np.sqrt(bn.var + EPS) * bn.gamma + bn.beta, 0).astype(np.float32))
    got = folded(c, bn, 1, None, True, True, True, False).float().cpu().numpy()
    np.testing.assert_allclose(got, yr, rtol=2.0 ** -7, atol=1e-5)


@pytest.mark.parametrize("K,n,cin,cout,pair", B_CASES)
def test_bf16_operand_kernel(K, n, cin, cout, pair):
    """conv_apply_b (BTC_OPERANDS_BF16), key 21 = the case's value, and 1 / 2 where the reduction is 32 channels"""
    from btcdet_amd._lib import check, ptr, stream_ptr
    c = Case(K * 5 + n, n, K, cin, cout, bf16=True, pairs_per_row=6.0)
    q = torch.empty((2, c.w.numel()), dtype=torch.bfloat16, device=dev())
    check(L().btc_weights_to_bf16(ptr(c.w), K, cin, cout, ptr(q[0]), ptr(q[1]), stream_ptr()), "btc_weights_to_bf16")
    with tuned((PAIR, pair)):
        same_bits(c, 2, q[1], what="conv_apply_b")
    if cin == 32:
        for pv in (1, 2):
            with tuned((PAIR, pv)):
                same_bits(c, 2, q[1], variants=VARIANTS[:2], what="conv_apply_b pair %d" % pv)


# ------------------------------------------------------------------ routing
def _net(cin=16, mid=32, cout=64, bias=False):
    from functools import partial
    from btcdet_amd import spconv
    torch.manual_seed(3)
    norm = partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)
    net = spconv.SparseSequential(
        spconv.SubMConv3d(cin, mid, 3, padding=1, bias=bias, indice_key="subm1"), norm(mid), torch.nn.ReLU(),
        spconv.SparseConv3d(mid, cout, 3, stride=2, padding=1, bias=bias, indice_key="spconv2"), norm(cout), torch.nn.ReLU()).to(dev())
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.3, 0.3)
    return net


def _input(n=3000, cin=16, dtype=torch.float32, indice_dict=None, requires_grad=False):
    from btcdet_amd import spconv
    rng = np.random.default_rng(5)
    idx = rand_indices(rng, n, 2, (10, 24, 20))
    feat = torch.from_numpy(rng.standard_normal((idx.shape[0], cin)).astype(np.float32)).to(dev()).to(dtype)
    feat.requires_grad_(requires_grad)
    x = spconv.SparseConvTensor(feat, _g(idx), [10, 24, 20], 2)
    if indice_dict is not None:
        x.indice_dict = indice_dict
    return x


class Counter:
    """calls of the fold's binding entry: the compiled binding counts its own (eval_fold_calls), the ctypes route is wrapped"""

    def __init__(self, monkeypatch):
        from btcdet_amd import _lib
        self.F, self.n_ctypes = _lib.fast(), 0
        lib = _lib.lib()
        inner = lib.btc_conv_bn_eval_fwd

        def counted(*a):
            self.n_ctypes += 1
            return inner(*a)
        monkeypatch.setattr(lib, "btc_conv_bn_eval_fwd", counted)
        self.mark()

    def mark(self):
        self.base = (self.F.eval_fold_calls() if self.F is not None else 0) + self.n_ctypes

    def delta(self):
        now = (self.F.eval_fold_calls() if self.F is not None else 0) + self.n_ctypes
        d, self.base = now - self.base, now
        return d


def _bn_state(net):
    return {k: v.clone() for k, v in net.state_dict().items()}


def test_routing_compiled_binding(monkeypatch):
    """an eval chain under no_grad folds (per-layer calls and the chain call), also with gradients enabled when nothing requires one;
    training mode, key 23 = 1 and an input that requires grad do not -- and then the gradients are today's bits"""
    from btcdet_amd import _lib
    assert _lib.fast() is not None, "the compiled binding is not built"
    cnt = Counter(monkeypatch)
    net = _net().eval()
    state = _bn_state(net)
    with torch.no_grad():
        y1 = net(_input())                                   # rulebooks are built on the way: one module call per layer
        assert cnt.delta() == 2 and cnt.n_ctypes == 0
        y2 = net(_input(indice_dict=y1.indice_dict))         # rulebooks at hand: SparseSequential._run_chain -> conv_bn_relu_chain
        assert cnt.delta() == 2
        with tuned((EVAL_FOLD, 1)):
            y3 = net(_input())
            y4 = net(_input(indice_dict=y3.indice_dict))
        assert cnt.delta() == 0
    for y in (y2, y3, y4):
        assert torch.equal(y.features, y1.features) and torch.equal(y.indices, y1.indices)
    assert not y1.features.requires_grad
    for k, v in net.state_dict().items():
        assert torch.equal(v, state[k]), k
    # gradients enabled, parameters frozen, input without grad: nothing will ask for a gradient -> folded
    for p in net.parameters():
        p.requires_grad_(False)
    y5 = net(_input())
    assert cnt.delta() == 2 and torch.equal(y5.features, y1.features) and not y5.features.requires_grad
    for p in net.parameters():
        p.requires_grad_(True)
    # eval mode WITH gradients (frozen-statistics fine-tuning): the autograd node, and its gradients bit for bit those of key 23 = 1
    grads = []
    for key in (0, 1):
        net.zero_grad(set_to_none=True)
        with tuned((EVAL_FOLD, key)):
            x = _input(requires_grad=True)
            y = net(x)
            assert cnt.delta() == 0
            assert torch.equal(y.features.detach(), y1.features)
            torch.manual_seed(1)
            y.features.backward(torch.randn_like(y.features))
            from btcdet_amd.spconv import ops
            ops.join_wgrad()
            torch.cuda.synchronize()
        grads.append([x.features.grad.clone()] + [p.grad.clone() for p in net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    # parameters that require grad, input that does not, gradients enabled: still the node
    y = net(_input())
    assert cnt.delta() == 0 and y.features.requires_grad
    # training mode never folds
    net.train()
    with torch.no_grad():
        net(_input())
    assert cnt.delta() == 0


@pytest.mark.parametrize("dtype,keys", [(torch.float32, ()), (torch.float32, ((SPLIT, 1),)), (torch.bfloat16, ()), (torch.bfloat16, ((BF16_OPERANDS, 1),))],
                         ids=["fp32", "fp32-exact", "bf16", "bf16-fp32-weights"])
def test_routing_both_bindings_agree(monkeypatch, dtype, keys):
    """BTC_FASTPATH=0 (the ctypes route) folds too, and both bindings give the same bits as today's three launches (key 23 = 1), with the
    split kernel allowed (6000 rows of 32 -> 64: it is taken) or not (key 14 = 1), bf16 operands or fp32 weights under bf16 (key 8 = 1)"""
    from btcdet_amd import _lib
    cnt = Counter(monkeypatch)
    net = _net(cin=32, mid=64, cout=64, bias=True).eval()
    outs = {}
    with torch.no_grad(), tuned(*keys):
        if dtype == torch.float32:
            assert (L().btc_conv_split_wanted(27, 32, 64, 9000) == 1) == (not keys)
        for binding in ("fast", "ctypes"):
            monkeypatch.setattr(_lib, "_fast", _lib._fast if binding == "fast" else None)
            assert (_lib.fast() is None) == (binding == "ctypes")
            for fold in (0, 1):
                with tuned((EVAL_FOLD, fold)):
                    c0 = cnt.n_ctypes
                    y = net(_input(n=9000, cin=32, dtype=dtype))
                    d = cnt.delta()
                    assert d == (2 if fold == 0 else 0), (binding, fold, d)
                    assert (cnt.n_ctypes - c0) == (2 if (fold == 0 and binding == "ctypes") else 0)
                    outs[(binding, fold)] = y.features
    ref = outs[("fast", 1)]
    assert ref.dtype == dtype and bool(torch.isfinite(ref.float()).all())
    for k, v in outs.items():
        assert torch.equal(v, ref), k


# ------------------------------------------------------------------ the whole eval forward
@pytest.mark.parametrize("features,heads", [("fp32", None), ("fp32", "full"), ("bf16", None), ("bf16", "full")])
def test_whole_eval_forward_is_unchanged_by_the_fold(monkeypatch, features, heads):
    """BtcHotPath in eval mode under no_grad: spatial_features, x_combine (and with heads="full" batch_cls_preds / batch_box_preds) are
    identical with key 23 = 0 and 1, layers are folded (counted), and no buffer or parameter moves.  (Measured while writing this: without
    the request for deterministic library algorithms below, torch's Conv1d of the ROI head's class branch moved 170-187 of the 200
    batch_cls_preds by 3-5e-8 from run to run, between two folded runs as much as between a folded and an unfolded one; rois,
    pooled_features and batch_box_preds were identical either way.)"""
    import bench
    from btcdet_amd.btc_path import BtcHotPath
    from btcdet_amd.config import load_cfg
    cfg = load_cfg()
    if features == "bf16":      # as bench.py --features bf16 sets them
        cfg.MODEL.OCC.BACKBONE_3D["FEATURE_DTYPE"] = "bf16"
        cfg.MODEL.BACKBONE_3D["FEATURE_DTYPE"] = "bf16"
    torch.manual_seed(0)
    np.random.seed(0)
    model = BtcHotPath(cfg, device=torch.device(dev()), heads=heads).to(dev())
    batches = bench.build_batches(2, 3, torch.device(dev()))
    model.train()
    with torch.no_grad():
        for b in batches:        # running statistics other than their initial values
            model(model.prepare(b))
    model.eval()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    cnt = Counter(monkeypatch)
    outs = []
    # torch's own layers of the ROI head (Conv1d through MIOpen / rocBLAS) may pick reductions with atomics, whose bits move from run to run
    # whatever key 23 says: ask the libraries for their deterministic algorithms, so that a difference below can only be the fold's
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    det = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        outs = _eval_runs(model, batches[0], heads, cnt)
    finally:
        torch.use_deterministic_algorithms(det[0], warn_only=det[1])
    _compare_runs(outs)
    for k, v in model.state_dict().items():
        assert torch.equal(v, state[k]), k


def _eval_runs(model, batch, heads, cnt):
    outs = []
    with torch.no_grad():
        for fold in (0, 1, 0):
            with tuned((EVAL_FOLD, fold)):
                out, _, bd = model(model.prepare(batch, is_train=False))
                torch.cuda.synchronize()
            n_folded = cnt.delta()
            assert (n_folded >= 20) if fold == 0 else (n_folded == 0), n_folded      # (27 conv -> BatchNorm layers on the hot path)
            keep = {"spatial_features": out["spatial_features"], "x_combine": out["x_combine"]}
            if heads == "full":
                keep.update(rois=bd["rois"], pooled_features=bd["pooled_features"], batch_cls_preds=bd["batch_cls_preds"], batch_box_preds=bd["batch_box_preds"])
            outs.append(keep)
    return outs


def _compare_runs(outs):
    for k in outs[0]:
        for a, b in ((0, 1), (0, 2), (1, 2)):
            x, y = outs[a][k].float(), outs[b][k].float()
            print("%s: runs %d / %d: %d of %d elements differ, max |diff| %.3g" % (k, a, b, int((x != y).sum()), x.numel(), float((x - y).abs().max())))
        assert bool(torch.isfinite(outs[0][k].float()).all()), k
        assert torch.equal(outs[0][k], outs[1][k]), k + ": fold on / off"
        assert torch.equal(outs[0][k], outs[2][k]), k + ": run to run"
