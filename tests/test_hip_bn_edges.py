"""The BatchNorm family of csrc/bn.hip (statistics, apply, their backward twins, btc_col_sum) and the statistics epilogue of
csrc/bn_fuse.h against the float64 reference and the derived bounds of tests/bn_ref.py, stage by stage, at the shapes where the
kernels branch: the scalar and the vector statistics path, channel-group counts that are no power of two, a second channel pass,
the unrolled row loops at their exact boundaries, one / two / capped grids and workgroups without rows, every combination of
absent parameters, eval (given-statistics) mode with gradients, bf16 activations, both bindings, dirty and shared workspaces.
The worst ratio |got - ref| / bound per stage is printed by the last test of the module."""
import numpy as np
import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-3, 0.01
CHANNELS = [1, 2, 3, 5, 4, 12, 20, 32, 34, 128, 150, 256, 257, 260, 1028, 1030]
BF16_CHANNELS = [4, 12, 32, 34, 260]
MODES = ["train_running", "train_null", "eval"]
W = R.Worst()


def dev():
    return torch.device("cuda:0")


def rows_per_iteration(c):
    """bn_shape of csrc/bn.hip: cpow = power of two >= min(c, 256), a workgroup of 256 threads walks rpi = 256 / cpow rows per
    iteration; on the vector path (C % 4 == 0) c is the number of 4-channel groups, C / 4"""
    cpow = 1
    while cpow < c and cpow < 256:
        cpow <<= 1
    return 256 // cpow


def row_counts(C):
    """the single-workgroup loop edges: the tail loop alone, the 2-deep and the 4-deep unrolled loop at their exact boundaries.
    The vector kernels walk with the rpi of C / 4; their last-arriver reduction and btc_col_sum walk with the rpi of C: both sets"""
    ns = set()
    for rpi in {rows_per_iteration(C // 4 if C % 4 == 0 else C), rows_per_iteration(C)}:
        ns |= {1, 2, 3, rpi - 1, rpi, rpi + 1, 4 * rpi - 1, 4 * rpi, 4 * rpi + 1, 9 * rpi + 2}
    return sorted(n for n in ns if n >= 1)


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Wrapper:
    """the Python entry points (compiled binding when built, else ctypes), on fused_bn's own workspace"""

    def fwd(self, x, g, b, rm, rv, nbt, training, relu):
        from btcdet_amd.spconv import fused_bn
        return fused_bn.bn_forward(x, g, b, rm, rv, nbt, training, MOM, EPS, relu)

    def bwd(self, x, y, dy, g, stats, training, relu):
        from btcdet_amd.spconv import fused_bn
        return fused_bn.bn_backward(x, y, dy, g, stats, training, relu)

    def col_sum(self, x):
        from btcdet_amd.spconv import fused_bn
        return fused_bn.col_sum(x)


class Abi:
    """the C ABI through ctypes with a workspace the test owns: the head (first 256 bytes) must be zero after every call"""

    def __init__(self, ws):
        self.ws = ws

    def _call(self, name, bf, *args):
        from btcdet_amd._lib import check, lib
        fn = getattr(lib(), name + ("_bf16" if bf else ""))
        check(fn(*args), name)
        assert int(self.ws[:256].count_nonzero()) == 0, f"{name}: workspace head not left zeroed"

    def fwd(self, x, g, b, rm, rv, nbt, training, relu):
        from btcdet_amd._lib import lib, ptr, stream_ptr
        n, c = x.shape
        y, stats = torch.empty_like(x), torch.empty((2, c), dtype=torch.float32, device=x.device)
        self._call("btc_bn_relu_fwd", x.dtype == torch.bfloat16, ptr(x), n, c, ptr(g), ptr(b), ptr(rm), ptr(rv), ptr(nbt), MOM, EPS, int(training),
                   int(relu), ptr(y), ptr(stats[0]), ptr(stats[1]), ptr(self.ws), lib().btc_bn_ws_bytes(c), stream_ptr())
        return y, stats

    def bwd(self, x, y, dy, g, stats, training, relu):
        from btcdet_amd._lib import lib, ptr, stream_ptr
        n, c = x.shape
        dx, dp = torch.empty_like(x), torch.empty((2, c), dtype=torch.float32, device=x.device)
        self._call("btc_bn_relu_bwd", x.dtype == torch.bfloat16, ptr(x), ptr(y), ptr(dy), n, c, ptr(g), ptr(stats[0]), ptr(stats[1]), int(training),
                   int(relu), ptr(dx), ptr(dp[0]), ptr(dp[1]), ptr(self.ws), lib().btc_bn_ws_bytes(c), stream_ptr())
        return dx, dp[0], dp[1]

    def col_sum(self, x):
        from btcdet_amd._lib import lib, ptr, stream_ptr
        n, c = x.shape
        out = torch.empty((c,), dtype=torch.float32, device=x.device)
        self._call("btc_col_sum", x.dtype == torch.bfloat16, ptr(x), n, c, ptr(out), ptr(self.ws), lib().btc_bn_ws_bytes(c), stream_ptr())
        return out


def up(a, dtype=torch.float32):
    return torch.from_numpy(a).to(dev()).to(dtype)


def run_case(api, n, c, seed, mode="train_running", relu=True, affine=True, bf16=False, check=True, dy_is_xhat=False):
    """one forward + backward + column sum, made twice from identical inputs: the two must agree bit for bit, and every stage must
    meet its bound.  -> the first call's tensors"""
    training, running = mode != "eval", mode != "train_null"
    d = R.make_inputs(n, c, seed, bf16)
    if dy_is_xhat:                                            # every term of dgamma = sum dy x-hat positive: nothing cancels along the sum
        d["dy"] = ((d["x"] - d["x"].mean(0)) / (d["x"].std(0) + 1e-3)).astype(np.float32)
    tdt = torch.bfloat16 if bf16 else torch.float32
    x, dy = up(d["x"], tdt), up(d["dy"], tdt)
    g, b = (up(d["gamma"]), up(d["beta"])) if affine else (None, None)
    where = f"N={n} C={c} {mode} relu={relu} affine={affine}"
    outs = []
    for _ in range(2):
        rm, rv = (up(d["running_mean"]), up(d["running_var"])) if running else (None, None)
        nbt = torch.full((), 5, dtype=torch.long, device=dev()) if (running and training) else None
        y, stats = api.fwd(x, g, b, rm, rv, nbt, training, relu)
        dx, dg, db = api.bwd(x, y, dy, g, stats, training, relu)
        o = dict(mean=stats[0], rstd=stats[1], y=y, dx=dx, dgamma=dg, dbeta=db, col_sum=api.col_sum(x))
        if running:
            o.update(running_mean=rm, running_var=rv)
        if nbt is not None:
            assert int(nbt) == 6, where                       # + 1 per call
        outs.append(o)
    for k in outs[0]:
        assert bits_equal(outs[0][k], outs[1][k]), f"{k} differs between two identical calls, {where}"
    assert y.dtype == tdt and dx.dtype == tdt and stats.dtype == torch.float32
    if check:
        got = {k: v.float().cpu().numpy() for k, v in outs[0].items()}
        if not training:                                      # eval reads the running statistics and leaves them alone
            assert np.array_equal(got.pop("running_mean"), d["running_mean"]) and np.array_equal(got.pop("running_var"), d["running_var"]), where
        R.check_all(W, "bf16" if bf16 else "fp32", d, got, training, relu, affine, bf16, MOM, EPS, where)
    return outs[0]


# ---- the single-workgroup loop edges of every channel-count branch, every mode
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", CHANNELS)
def test_loop_edges(C, mode, relu):
    for n in row_counts(C):
        run_case(Wrapper(), n, C, 1000 * C + n, mode, relu)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", BF16_CHANNELS)
def test_loop_edges_bf16(C, mode, relu):
    for n in row_counts(C):
        run_case(Wrapper(), n, C, 1000 * C + n + 500000, mode, relu, bf16=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [5, 12, 260])
def test_without_gamma_and_beta(C, mode):
    for n in row_counts(C):
        run_case(Wrapper(), n, C, 1000 * C + n + 7, mode, True, affine=False)


def test_single_row_in_training():
    """N = 1, which torch refuses: mean = x, variance 0, rstd = 1 / sqrt(eps), the running variance decays only (the table of
    tests/bn_ref.py is the statement of record); y = beta, dx = 0 up to rounding"""
    for C in (5, 32, 260):
        o = run_case(Wrapper(), 1, C, 77 + C, "train_running", False)
        d = R.make_inputs(1, C, 77 + C)
        np.testing.assert_array_equal(o["mean"].cpu().numpy(), d["x"][0])
        np.testing.assert_array_equal(o["rstd"].cpu().numpy(), np.float32(1.0 / np.sqrt(R.f32(EPS))))
        np.testing.assert_array_equal(o["y"].cpu().numpy()[0], d["beta"])


def test_num_batches_tracked_counts_calls():
    d = R.make_inputs(300, 12, 3)
    x, rm, rv = up(d["x"]), up(d["running_mean"]), up(d["running_var"])
    nbt = torch.zeros((), dtype=torch.long, device=dev())
    for k in range(1, 4):
        Wrapper().fwd(x, None, None, rm, rv, nbt, True, True)
        assert int(nbt) == k
    Wrapper().fwd(x, None, None, rm, rv, None, False, True)   # eval: no count
    assert int(nbt) == 3


# ---- grids: one -> two workgroups, the capped grids, workgroups that receive no rows
@pytest.mark.parametrize("n,c", [(511, 32), (512, 32), (513, 32),   # forward: 64 KiB per workgroup, 1 -> 2 workgroups
                                 (341, 32), (342, 32),              # backward: 128 KiB over 12 B per element
                                 (131073, 32),                      # both vector grids capped at 256
                                 (526337, 5)])                      # scalar forward grid capped at 256, backward and col_sum at 512
def test_grid_edges(n, c):
    run_case(Wrapper(), n, c, n + c)


@pytest.mark.parametrize("n,c", [(700, 128), (700, 34)])
@pytest.mark.parametrize("value", [1, 4096])
@pytest.mark.parametrize("key", [9, 10])
def test_tuned_grids_meet_the_same_bounds(key, value, n, c):
    """BTC_TUNE_BN_FWD_KB / BTC_TUNE_BN_BWD_KB: at 1 KiB per workgroup most of the 256 workgroups own no rows, at 4096 one owns all"""
    from btcdet_amd._lib import check, lib
    check(lib().btc_tune_set(key, value), "btc_tune_set")
    try:
        run_case(Wrapper(), n, c, 10 * key + value + c)
    finally:
        check(lib().btc_tune_set(key, 0), "btc_tune_set")


@pytest.mark.parametrize("n,c", [(700, 128), (9 * 64 + 2, 4)])
def test_tuned_grids_bf16(n, c):
    from btcdet_amd._lib import check, lib
    for key in (9, 10):
        check(lib().btc_tune_set(key, 1), "btc_tune_set")
    try:
        run_case(Wrapper(), n, c, n + c + 1, bf16=True)
    finally:
        for key in (9, 10):
            check(lib().btc_tune_set(key, 0), "btc_tune_set")


def test_one_workgroup_walks_every_row():
    """BTC_TUNE_BN_FWD_KB / BTC_TUNE_BN_BWD_KB = 64 MiB per workgroup on a 4096 x 1028 layer: ONE workgroup, and with 257 channel
    groups rpi = 1, so each thread sums all 4096 rows of its channels by itself -- the longest chain of additions the kernels can
    be given (the built-in policy keeps a thread's chain to a few dozen rows and adds the chains up in fp64, which is why an fp32
    accumulator inside a thread is invisible at every other shape of this file).  With dy = x-hat the terms of dgamma are all
    positive: an fp32 accumulator then loses about 2^-24 |sum| per addition, several times the bound at this N (3 to 6 in a numpy emulation); fp64 stays at a tenth"""
    from btcdet_amd._lib import check, lib
    for key in (9, 10):
        check(lib().btc_tune_set(key, 65536), "btc_tune_set")
    try:
        run_case(Wrapper(), 4096, 1028, 4, relu=False, dy_is_xhat=True)
    finally:
        for key in (9, 10):
            check(lib().btc_tune_set(key, 0), "btc_tune_set")


# ---- workspace contract through the C ABI
WS_SHAPES = {260: 1203, 5: 5003, 32: 1501}      # several workgroups each (vector: bytes per workgroup; scalar: 64 rows per thread-row)


def _ws(nbytes):
    return torch.zeros(int(nbytes), dtype=torch.uint8, device=dev())


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 32, 260])
def test_dirty_workspace_tail_changes_nothing(C, bf16):
    """head zero on entry and after each call; whatever the rest holds (here NaN patterns) the results are the clean workspace's bits"""
    from btcdet_amd._lib import lib
    if bf16 and C == 5:
        C = 34
    n = WS_SHAPES.get(C, 1501)
    need = lib().btc_bn_ws_bytes(C)
    clean = run_case(Abi(_ws(need)), n, C, 31 + C, bf16=bf16)
    ws = _ws(need)
    ws[256:] = 0xFF
    dirty = run_case(Abi(ws), n, C, 31 + C, bf16=bf16, check=False)
    for k in clean:
        assert bits_equal(clean[k], dirty[k]), k


def test_one_workspace_shared_by_layers_of_different_width():
    """C = 260, then 5, then 32 on one workspace: partial sums of a wider layout must not leak into a narrower one"""
    from btcdet_amd._lib import lib
    shared = _ws(lib().btc_bn_ws_bytes(260))
    for C in (260, 5, 32):
        clean = run_case(Abi(_ws(lib().btc_bn_ws_bytes(C))), WS_SHAPES[C], C, 57 + C, check=False)
        again = run_case(Abi(shared), WS_SHAPES[C], C, 57 + C)
        for k in clean:
            assert bits_equal(clean[k], again[k]), (C, k)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_workspace_one_byte_short_is_refused(bf16):
    from btcdet_amd._lib import lib, ptr, stream_ptr
    L = lib()
    n, c = 300, 12
    tdt = torch.bfloat16 if bf16 else torch.float32
    d = R.make_inputs(n, c, 5, bf16)
    x, dy = up(d["x"], tdt), up(d["dy"], tdt)
    need = L.btc_bn_ws_bytes(c)
    ws = _ws(need)
    sfx = "_bf16" if bf16 else ""
    y, dx = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    stats, dp, cs = (torch.full((2, c), 7.0, device=dev()) for _ in range(3))
    calls = {
        "btc_bn_relu_fwd": lambda: getattr(L, "btc_bn_relu_fwd" + sfx)(ptr(x), n, c, None, None, None, None, None, MOM, EPS, 1, 1, ptr(y), ptr(stats[0]),
                                                                      ptr(stats[1]), ptr(ws), need - 1, stream_ptr()),
        "btc_bn_relu_bwd": lambda: getattr(L, "btc_bn_relu_bwd" + sfx)(ptr(x), ptr(x), ptr(dy), n, c, None, ptr(stats[0]), ptr(stats[1]), 1, 1, ptr(dx),
                                                                      ptr(dp[0]), ptr(dp[1]), ptr(ws), need - 1, stream_ptr()),
        "btc_col_sum": lambda: getattr(L, "btc_col_sum" + sfx)(ptr(x), n, c, ptr(cs[0]), ptr(ws), need - 1, stream_ptr()),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = L.btc_last_error().decode()
        assert name in msg and "workspace" in msg, msg
    torch.cuda.synchronize()
    for t in (y, dx, stats, dp, cs):                          # no launch: nothing written
        assert bool((t == 7.0).all())
    assert int(ws.count_nonzero()) == 0


# ---- both bindings
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [5, 32, 260])
def test_compiled_and_ctypes_binding_give_the_same_bits(C, bf16):
    from btcdet_amd import _lib
    if bf16 and C == 5:
        C = 34
    if _lib.fast() is None:
        pytest.skip("the compiled binding is not built; the ctypes route is covered by the workspace tests")
    n = WS_SHAPES.get(C, 1501)
    for mode in MODES:
        fast_res = run_case(Wrapper(), n, C, 91 + C, mode, bf16=bf16)
        saved = _lib._fast
        _lib._fast = None  # force the ctypes route
        try:
            ct_res = run_case(Wrapper(), n, C, 91 + C, mode, bf16=bf16, check=False)
        finally:
            _lib._fast = saved
        for k in fast_res:
            assert bits_equal(fast_res[k], ct_res[k]), (mode, k)


# ---- the autograd wrapper, end to end against torch's float64 module
E2E_VARIANTS = ["plain", "no_affine", "no_running_stats", "eval_with_grad", "non_contiguous"]


@pytest.mark.parametrize("variant", E2E_VARIANTS)
@pytest.mark.parametrize("n,c", [(37, 5), (513, 12), (1000, 260)])
def test_batch_norm_relu_node_matches_torch_float64(n, c, variant):
    """fused_bn.batch_norm_relu on an nn.BatchNorm1d, forward and backward, at the tolerances of test_fused_batchnorm_relu_matches_torch"""
    from btcdet_amd.spconv import fused_bn
    torch.manual_seed(n + c)
    affine, track, training = variant != "no_affine", variant != "no_running_stats", variant != "eval_with_grad"
    bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=MOM, affine=affine, track_running_stats=track).to(dev())
    with torch.no_grad():
        if affine:
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
        if track:
            bn.running_mean.uniform_(-0.1, 0.1)
            bn.running_var.uniform_(0.5, 1.5)
    ref = torch.nn.BatchNorm1d(c, eps=EPS, momentum=MOM, affine=affine, track_running_stats=track).to(dev()).double()
    ref.load_state_dict({k: (v.double() if v.is_floating_point() else v.clone()) for k, v in bn.state_dict().items()})
    bn.train(training)
    ref.train(training)
    full = torch.randn(n, c + 3, device=dev()) * 2 + 0.5
    g = torch.randn(n, c, device=dev())
    if variant == "non_contiguous":
        leaf = full.clone().requires_grad_(True)
        xa = leaf[:, 1:1 + c]
        assert not xa.is_contiguous()
    else:
        leaf = full[:, 1:1 + c].contiguous().requires_grad_(True)
        xa = leaf
    ya = fused_bn.batch_norm_relu(bn, xa, True)
    ya.backward(g)
    dxa = leaf.grad[:, 1:1 + c] if variant == "non_contiguous" else leaf.grad
    xb = full[:, 1:1 + c].double().clone().requires_grad_(True)
    yb = torch.relu(ref(xb))
    yb.backward(g.double())
    tol = dict(rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(ya.detach().cpu().numpy(), yb.detach().cpu().numpy(), **tol)
    np.testing.assert_allclose(dxa.cpu().numpy(), xb.grad.cpu().numpy(), rtol=2e-4, atol=2e-5)
    if affine:
        np.testing.assert_allclose(bn.weight.grad.cpu().numpy(), ref.weight.grad.cpu().numpy(), rtol=2e-4, atol=2e-3)
        np.testing.assert_allclose(bn.bias.grad.cpu().numpy(), ref.bias.grad.cpu().numpy(), rtol=2e-4, atol=2e-3)
    else:
        assert bn.weight is None and bn.bias is None
    if track:
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), ref.running_mean.cpu().numpy(), **tol)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), ref.running_var.cpu().numpy(), **tol)
        assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == int(training)
    else:
        assert bn.running_mean is None and bn.num_batches_tracked is None


@pytest.mark.parametrize("n,c", [(37, 5), (513, 12), (1000, 260)])
def test_float32_gradient_into_a_bf16_node(n, c):
    """a float32 dy arriving at a node whose activations are bf16 is the bf16-rounded dy: same bits, bf16 dx, fp32 parameter gradients"""
    from btcdet_amd.spconv import fused_bn
    torch.manual_seed(n + c)
    x = (torch.randn(n, c, device=dev()) * 2 + 0.5).to(torch.bfloat16)
    g = torch.randn(n, c, device=dev())
    res = []
    for dy in (g, g.to(torch.bfloat16)):
        bn = torch.nn.BatchNorm1d(c, eps=EPS, momentum=MOM).to(dev())
        xa = x.clone().requires_grad_(True)
        ya = fused_bn.batch_norm_relu(bn, xa, True)
        assert ya.dtype == torch.bfloat16
        ya.backward(dy)
        res.append((xa.grad, bn.weight.grad, bn.bias.grad))
    assert res[0][0].dtype == torch.bfloat16 and res[0][1].dtype == torch.float32 and res[0][2].dtype == torch.float32
    for a, b in zip(*res):
        assert bits_equal(a, b)
    y32 = torch.relu(torch.nn.functional.batch_norm(x.float(), None, None, bn.weight.detach(), bn.bias.detach(), True, 0.0, EPS))
    assert float((ya.detach().float() - y32).abs().max()) <= 2.0 ** -8 * float(y32.abs().max()) + 2e-5


def test_no_rows_raises():
    from btcdet_amd.spconv import fused_bn
    bn = torch.nn.BatchNorm1d(5, eps=EPS, momentum=MOM).to(dev())
    with pytest.raises(Exception, match="empty input"):
        fused_bn.batch_norm_relu(bn, torch.empty((0, 5), device=dev()), True)
    assert int(bn.num_batches_tracked) == 0


# ---- wide results through the statistics epilogue of the sparse conv (csrc/bn_fuse.h: more channels than the workgroup has threads)
def rand_indices(rng, n, batch, shape):
    vol = int(np.prod(shape))
    lin = rng.choice(batch * vol, size=min(n, batch * vol), replace=False)
    b, rem = lin // vol, lin % vol
    z, rem = rem // (shape[1] * shape[2]), rem % (shape[1] * shape[2])
    return np.stack([b, z, rem // shape[2], rem % shape[2]], axis=1).astype(np.int32)


@pytest.mark.parametrize("cout", [256, 272, 512, 1024, 1040])
def test_conv_epilogue_statistics_of_wide_layers(cout):
    """btc_conv_bn_relu_fwd with 256 .. 1024 result channels (statistics in the conv epilogue) and 1040 (the separate pass): the
    conv result does not depend on where the statistics are taken; mean / rstd / running statistics / y meet the bounds of
    tests/bn_ref.py with the reference taken from the conv result the call returns; the slot buffer is left zeroed"""
    from btcdet_amd import _lib
    from btcdet_amd.spconv import fused_bn, ops
    L = _lib.lib()
    rng = np.random.default_rng(cout)
    shape, B, cin = (8, 30, 36), 2, 16
    idx = rand_indices(rng, 700, B, shape)
    rb = ops.build_rulebook(torch.from_numpy(idx).to(dev()), B, shape, 3, 1, 1, 1, 0, True, False)
    m = rb.nbr_out.shape[0]
    assert m == 700 and rb.nbr_out.shape[1] == 27
    feat = up(rng.standard_normal((m, cin)).astype(np.float32))
    w = up((rng.standard_normal((27, cin, cout)) / np.sqrt(cin)).astype(np.float32))
    d = dict(gamma=rng.uniform(0.5, 1.5, cout).astype(np.float32), beta=rng.uniform(-0.5, 0.5, cout).astype(np.float32),
             running_mean=rng.uniform(-0.1, 0.1, cout).astype(np.float32), running_var=rng.uniform(0.5, 1.5, cout).astype(np.float32))
    gamma, beta = up(d["gamma"]), up(d["beta"])
    outs = []
    for tune in (0, 1, 0):
        rm, rv = up(d["running_mean"]), up(d["running_var"])
        nbt = torch.zeros((), dtype=torch.long, device=dev())
        assert L.btc_tune_set(12, tune) == 0
        try:
            x, y, stats = fused_bn.conv_bn_forward(feat, w, None, rb.nbr_out, None, gamma, beta, rm, rv, nbt, MOM, EPS, True)
            torch.cuda.synchronize()
        finally:
            L.btc_tune_set(12, 0)
        assert int(nbt) == 1
        assert bool((fused_bn.fuse_ws(feat.device) == 0).all())                  # slots and counter left zeroed
        outs.append((x, y, stats, rm, rv))
    assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][0], outs[2][0])
    xs = outs[0][0].cpu().numpy()
    assert np.isfinite(xs).all() and float(np.abs(xs).max()) > 0.1
    for i, (x, y, stats, rm, rv) in enumerate(outs):
        where = f"cout={cout} run {i}"
        W.check("mean", "fp32", stats[0].cpu().numpy(), R.mean(xs), where)
        W.check("rstd", "fp32", stats[1].cpu().numpy(), R.rstd(xs, EPS), where)
        rmr, rvr = R.running(xs, d["running_mean"], d["running_var"], MOM, EPS)
        W.check("running_mean", "fp32", rm.cpu().numpy(), rmr, where)
        W.check("running_var", "fp32", rv.cpu().numpy(), rvr, where)
        W.check("y", "fp32", y.cpu().numpy(), R.y(xs, stats[0].cpu().numpy(), stats[1].cpu().numpy(), d["gamma"], d["beta"], True), where)


def test_report_worst_ratios(capsys):
    """last in the file: the worst ratio to its bound per stage, fp32 and bf16, over everything the tests above checked"""
    assert all(r <= 1.0 for r in W.worst.values())
    with capsys.disabled():
        print("\n" + W.report())
