"""The weight gradient's planner on the host (csrc/conv_wgrad.hip wgrad_max_slabs, no GPU): btc_conv_wgrad_ws_bytes over a grid of
shapes equals the values recorded in tests/golden/wgrad_ws_bytes.json, exactly.

The size is the largest slab count of every family's plan (the work splits of conv_wgrad_rows_p / _rows / conv_wgrad_x, the offset-major
split, conv_wgrad_n's) times K Cin Cout floats, so a plan that moves -- another tile row, another PH, another S -- moves a value here.
The grid crosses every row-count threshold (2048, 4096, the 3 x 512 (tile, group, block) triples that keep the full PH), K past 64, and
reaches every row of the tile tables; the three tuning keys that enter the sizing (5 = PH, 6 = workgroups, 11 = the two-barrier kernels)
run over every fourth point."""
import json
import os

N_OUT = [0, 1, 64, 129, 2047, 2048, 4095, 4096, 4160, 12000, 49152, 210000]
N_IN = [lambda n: -1, lambda n: n, lambda n: n // 8]
KS = [1, 3, 27, 64, 65, 125]
CHANNELS = [(4, 16), (6, 16), (16, 16), (16, 32), (32, 16), (32, 32), (48, 32), (32, 64), (64, 32), (64, 64), (128, 128), (256, 128), (32, 5), (64, 3),
            (20, 48), (34, 32)]
KEYED = [(11, 1), (6, 256), (5, 2)]   # BTC_TUNE_WGRAD_PIPE, _WGS, _PH: over every fourth point of the grid
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_ws_bytes.json")


def _points():
    return [(n, f(n), K, cin, cout) for n in N_OUT for f in N_IN for K in KS for cin, cout in CHANNELS]


def ws_bytes_over_the_grid():
    """the whole grid at default keys, then every fourth point under each key of KEYED: a flat list in iteration order"""
    from btcdet_amd import _lib
    L = _lib.lib()
    size = lambda p: int(L.btc_conv_wgrad_ws_bytes(p[0], p[2], p[3], p[4], p[1]))
    pts = _points()
    out = [size(p) for p in pts]
    for key, value in KEYED:
        try:
            assert L.btc_tune_set(key, value) == 0
            out += [size(p) for p in pts[::4]]
        finally:
            assert L.btc_tune_set(key, 0) == 0
    return out


def test_workspace_sizes_equal_the_recorded_plans():
    want = json.load(open(GOLDEN))
    got = ws_bytes_over_the_grid()
    pts = _points()
    assert len(want) == len(got) == len(pts) + len(KEYED) * len(pts[::4])
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]

    def name(i):
        if i < len(pts):
            return "default keys", pts[i]
        j = i - len(pts)
        return "key %d = %d" % KEYED[j // len(pts[::4])], pts[::4][j % len(pts[::4])]
    assert not bad, "%d sizes moved; first: %s (n_out, n_in, K, Cin, Cout) = %s: %d, recorded %d" % (
        (len(bad),) + name(bad[0]) + (got[bad[0]], want[bad[0]]))
    assert len(set(want)) > 100          # (the grid does reach many different plans)
