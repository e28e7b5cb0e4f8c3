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
