"""CPU-side guards of the second public header, include/btcdet_hip_infer.h: the library exports every name it declares, the second
ctypes signature table (_lib._INFER_SIGS) equals it, the two headers share no name, and the argument checks of the new entry points
return an error code before any launch (no GPU is touched here)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_symbol_of_the_inference_header():
    from btcdet_amd import _lib
    L = _lib.lib()
    names = _declared("btcdet_hip_infer.h")
    assert names, "include/btcdet_hip_infer.h declares nothing"
    for n in names:
        assert hasattr(L, n), "libbtcdet_hip.so does not export %s" % n
    assert sorted(_lib.INFER_EXPORTED_SYMBOLS) == names, "second ctypes signature table and include/btcdet_hip_infer.h disagree"
    assert not set(names) & set(_declared("btcdet_hip.h")), "a name is declared in both headers"
    assert not set(names) & set(_lib.EXPORTED_SYMBOLS)
    for n in names:       # every signature was applied when the library was loaded
        fn = getattr(L, n)
        assert fn.argtypes == _lib._INFER_SIGS[n][1] and fn.restype == _lib._INFER_SIGS[n][0], n


def test_eval_fold_key_is_defined_free_and_documented():
    """BTC_TUNE_EVAL_FOLD is key 23 of 24, no other key has that number, and INTEGRATION section 7 lists it"""
    from btcdet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "btcdet_hip.h")).read()
    keys = re.findall(r"^#define (BTC_TUNE_[A-Z0-9_]+) (\d+)", hdr, flags=re.M)
    assert ("BTC_TUNE_EVAL_FOLD", "23") in keys
    assert [k for k, v in keys if v == "23"] == ["BTC_TUNE_EVAL_FOLD"]
    L = _lib.lib()
    try:
        assert L.btc_tune_set(23, 1) == 0 and L.btc_tune_value(23) == 1
    finally:
        assert L.btc_tune_set(23, 0) == 0
    assert L.btc_tune_set(24, 1) != 0       # BTC_TUNE_KEYS stays 24
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [ln for ln in doc.splitlines() if ln.startswith("| 23 |")]
    assert len(row) == 1 and "BTC_TUNE_EVAL_FOLD" in row[0] and "test_hip_eval_fold.py" in row[0]


def test_eval_fold_argument_checks_return_before_any_launch():
    """n_rows == 0, an unknown operand kind, missing running statistics, K past BTC_CONV_K_MAX, more than 1024 channels and split
    operands without the source's row count are BTC_EINVAL with a message; the (never dereferenced) pointers are not device memory"""
    from btcdet_amd import _lib
    L = _lib.lib()
    p = 0x1000      # a non-null address nobody reads: every call below returns from its argument checks

    def call(operands=0, src_rows=10, n_rows=10, K=27, cin=16, cout=16, rm=p, rv=p, src=p):
        return L.btc_conv_bn_eval_fwd(operands, src, src_rows, p, None, p, None, n_rows, K, cin, cout, None, None, rm, rv, 1e-3, 1, p, None)

    assert call(n_rows=0) == -1 and b"empty input" in L.btc_last_error()
    assert call(operands=4) == -1 and b"operands=4" in L.btc_last_error()
    assert call(operands=-1) == -1
    assert call(rm=None) == -1 and b"running statistics" in L.btc_last_error()
    assert call(rv=None) == -1 and b"running statistics" in L.btc_last_error()
    assert call(src=None) == -1
    assert call(K=513) == -1 and b"BTC_CONV_K_MAX = 512" in L.btc_last_error()
    assert call(cout=1040) == -1 and b"1024" in L.btc_last_error()
    assert call(operands=3, src_rows=-1, cin=32, cout=32) == -1 and b"row count of src" in L.btc_last_error()
    assert call(operands=2, cin=16, cout=16) == -1 and b"bf16 operands need" in L.btc_last_error()
