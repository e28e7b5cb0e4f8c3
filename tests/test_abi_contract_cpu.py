"""Completeness of the buffer-contract suite (tests/test_hip_abi_contract.py), on the CPU: every entry point include/btcdet_hip.h
declares is either called by a case of abi_contract.CASES or exempt below as a host-only function, and every case has its test."""
import ast
import os

from abi_contract import CASES
from test_abi_cpu import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# host-only functions: they enqueue no device work and write no device buffer
EXEMPT = {
    "btc_last_error": "host string of the last error",
    "btc_version": "host constant",
    "btc_tune_set": "host tuning registry",
    "btc_tune_value": "host tuning registry",
    "btc_out_shape": "host arithmetic on host arrays (tests/test_abi_cpu.py)",
    "btc_voxelize_ws_bytes": "host size query",
    "btc_range_mask_ws_bytes": "host size query",
    "btc_rulebook_subm_ws_bytes": "host size query",
    "btc_rulebook_conv_ws_bytes": "host size query",
    "btc_chain_ws_bytes": "host size query",
    "btc_chain_caps": "host capacities of the chain's levels (host arrays only)",
    "btc_pairs_from_nbr_ws_bytes": "host size query",
    "btc_conv_wgrad_ws_bytes": "host size query",
    "btc_conv_bf16w_supported": "host policy query",
    "btc_conv_split_supported": "host policy query",
    "btc_conv_split_wanted": "host policy query",
    "btc_set_scratch": "host registry of a caller-owned buffer; writes nothing",
    "btc_adam_max_segments": "host constant",
    "btc_adam_group_ws_bytes": "host size query",
    "btc_sumsq2_ws_bytes": "host size query",
    "btc_revoxelize_ws_bytes": "host size query",
    "btc_occ_targets_ws_bytes": "host size query",
    "btc_bn_ws_bytes": "host size query",
    "btc_bn_fuse_ws_bytes": "host size query",
    "btc_pass_occ_vox_ws_bytes": "host size query",
    "btc_occ_loss_ws_bytes": "host size query",
    "btc_nms_ws_bytes": "host size query",
    "btc_nms_topk_ws_bytes": "host size query",
    "btc_spin": "an idle wave for stream probing: reads and writes no buffer",
}


def _gpu_case_functions():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_hip_abi_contract.py")).read())
    return {n.name[len("case_"):] for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("case_")}


def test_every_declared_entry_point_has_a_contract_case_or_is_host_only():
    declared = set(declared_symbols())
    covered = {s for names in CASES.values() for s in names}
    assert not covered - declared, "cases name entry points the header does not declare: %s" % sorted(covered - declared)
    assert not set(EXEMPT) - declared, "exempt names the header does not declare: %s" % sorted(set(EXEMPT) - declared)
    assert not covered & set(EXEMPT), "both covered and exempt: %s" % sorted(covered & set(EXEMPT))
    missing = declared - covered - set(EXEMPT)
    assert not missing, "entry points without a contract case: %s" % sorted(missing)


def test_exempt_entry_points_take_no_stream():
    """a host-only function has no `void* stream` parameter (btc_spin only idles on it, btc_set_scratch keys its registry by it)"""
    import re
    src = open(os.path.join(ROOT, "include", "btcdet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in EXEMPT:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        if name not in ("btc_spin", "btc_set_scratch"):
            assert "stream" not in m.group(1), "%s takes a stream: it is not host-only" % name


def test_every_case_has_a_gpu_test():
    fns = _gpu_case_functions()
    assert set(CASES) == fns, "cases without a test: %s; tests without a case: %s" % (sorted(set(CASES) - fns), sorted(fns - set(CASES)))


P = 0x1000      # a non-null address nobody reads: every call below returns from its argument checks


def test_range_mask_argument_checks_return_before_any_launch():
    import ctypes
    import numpy as np
    from btcdet_amd import _lib
    L = _lib.lib()
    lim = np.array([0.0, -40.0, 70.4, 40.0], np.float32)

    def call(pts=P, pts_b=P, n=300, ld=4, ld_b=4, offs=P, batch=2, rng=lim, out=P, out_b=P, out_offs=P, keep_idx=None, ws=P, ws_bytes=1 << 20):
        h = rng if rng is None else _lib.f32p(np.ascontiguousarray(rng, dtype=np.float32))
        return L.btc_range_mask_compact(pts, pts_b, n, ld, ld_b, offs, batch, h, out, out_b, out_offs, keep_idx, ws, ws_bytes, None)
    for kw in ("offs", "rng", "out_offs", "ws"):
        assert call(**{kw: None}) == -1 and b"missing pointer (scene_offsets, h_range_xyxy, out_offsets or ws)" in L.btc_last_error(), kw
    for kw in ("pts", "out"):
        assert call(**{kw: None}) == -1 and b"missing pointer (points or out)" in L.btc_last_error(), kw
    assert call(out_b=None) == -1 and b"second array needs its output and row length" in L.btc_last_error()
    assert call(ld_b=0) == -1 and b"second array needs its output and row length" in L.btc_last_error()
    # the refusals from before the pointer checks keep their messages
    for kw in ({"ld": 1}, {"ld": 0}, {"batch": 0}, {"batch": -1}, {"n": -1}):
        assert call(**kw) == -1 and b"need n >= 0, ld >= 2 (x, y columns), batch >= 1" in L.btc_last_error(), kw
    need = L.btc_range_mask_ws_bytes(300)
    for ws_bytes in (0, 8, need - 1):
        assert call(ws_bytes=ws_bytes) == -1 and b"workspace too small" in L.btc_last_error(), ws_bytes
    for rng in ([1.0, 0.0, 0.5, 2.0], [0.0, 3.0, 1.0, 2.0]):
        assert call(rng=rng) == -1 and b"empty range" in L.btc_last_error(), rng
    assert ctypes.sizeof(ctypes.c_float) * 4 == lim.nbytes
