"""The bits of the weight gradient, case by case: one line per case with the slab count btc_conv_wgrad_slabs reports and the sha256 of
dW (two-call form, reduced by btc_wgrad_reduce_multi).  Run it in two builds and diff the outputs: a difference in n_slabs points at
the work split, a difference in bits with equal n_slabs at the instance that was launched or its arguments.

Cases: every row of tests/test_hip_wgrad_launch.py LAUNCH_CASES, the ROWS_P list of tests/test_hip_conv_kernel_volumes.py (fp32-pipe
families, both phase counts) and SHAPES x rulebook kinds of tests/test_hip_wgrad_x.py, each with fp32 and bf16 activations.  All inputs
come from numpy generators with fixed seeds."""
import ctypes, hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import test_hip_wgrad_x as tx
from test_hip_conv_kernel_volumes import NARROW, ROWS_P, WGRAD_PH, WGRAD_X, Case, tuned
from test_hip_wgrad_launch import LAUNCH_CASES, make_case, wgrad_both_forms
from btcdet_amd._lib import check, lib, ptr, stream_ptr


def line(what, dw, n_slabs):
    torch.cuda.synchronize()
    print("%-52s slabs %4d  %s" % (what, n_slabs, hashlib.sha256(dw.cpu().numpy().tobytes()).hexdigest()), flush=True)


def rulebook_case(rb, feat, dout, cin, cout):
    """tests/test_hip_wgrad_x.py _wgrad, two-call form, reduced"""
    dw, ws, n = tx._wgrad(feat, dout, rb, cin, cout, slabs=True)
    P, D = (ctypes.c_void_p * 1)(ptr(ws)), (ctypes.c_void_p * 1)(ptr(dw))
    if n >= 1:
        check(lib().btc_wgrad_reduce_multi(P, D, (ctypes.c_int * 1)(n), (ctypes.c_longlong * 1)(dw.numel()), 1, stream_ptr()), "reduce_multi")
    return dw, n


for bf16 in (False, True):
    dt = "bf16" if bf16 else "fp32"
    for family, cin, cout, K, rows, keys in LAUNCH_CASES:
        c = make_case(family, cin, cout, K, rows, bf16)
        with tuned(*keys):
            one, two, n, _ = wgrad_both_forms(c, family == "n_result_mirrored")
        line("%s %d->%d K %d %d rows %s" % (family, cin, cout, K, rows, dt), two, n)
    for cin, cout, K, rows in ROWS_P:
        rows = max(rows, 4096)
        c = Case(cin + K + rows, rows, K, cin, cout, bf16=bf16, pairs_per_row=4.0)
        full_ph = {(16, 16): 4, (32, 32): 8, (64, 64): 4, (32, 64): 4, (64, 32): 8}[(cin, cout)]
        for ph in (0, full_ph, full_ph // 2):
            with tuned((WGRAD_X, 1), (NARROW, 1), (WGRAD_PH, ph)):
                one, two, n, _ = wgrad_both_forms(c)
            line("ROWS_P %d->%d K %d %d rows key 5 = %d %s" % (cin, cout, K, rows, ph, dt), two, n)
    for kind, n_vox in [("subm", 9000), ("subm", 60000), ("conv", 30000), ("transpose", 5000)]:
        for cin, cout in tx.SHAPES:
            rng = np.random.default_rng(cin * 131 + cout + n_vox)
            rb, feat, dout = tx._case(rng, cin, cout, kind, n_vox, (6, 30, 28) if kind == "transpose" else (12, 48, 44))
            if bf16:
                feat, dout = feat.to(torch.bfloat16), dout.to(torch.bfloat16)
            with tuned((NARROW, 1)):
                dw, n = rulebook_case(rb, feat, dout, cin, cout)
            line("SHAPES %d->%d %s %d voxels %s" % (cin, cout, kind, n_vox, dt), dw, n)
