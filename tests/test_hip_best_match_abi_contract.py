"""The buffer contract of btc_place_templates (include/btcdet_hip_bestmatch.h), as the other contract files hold their entry points to
it: `out` is a Guarded buffer (poisoned payload between two guard bands) with spare rows past n_out, the call runs on a side stream.
Afterwards rows [0, n_out) are fully overwritten and equal the numpy restatement, rows past n_out and the guards are untouched, the
inputs hold the bits they held, and the same call on the current stream gives the same bits.  Garbage in bm_first / bm_rows moves
no write.  Refused arguments write nothing."""
import numpy as np
import pytest
import torch

import abi_contract as ac
import best_match_cases as bc
import test_hip_best_match as T

pytestmark = pytest.mark.gpu
SPARE = 5          # rows of capacity beyond n_out: there is always a row past it


def L():
    from btcdet_amd import _lib
    return _lib.lib()


def _case(sizes):
    """two scenes over the templates `sizes` (the first half in scene 0) -> host arrays"""
    rng = np.random.default_rng(sum(sizes) + len(sizes))
    bank = rng.uniform(-2, 2, (max(sum(sizes), 1) + 7, 3)).astype(np.float32)
    first = np.concatenate([[3], 3 + np.cumsum(sizes)[:-1]]).astype(np.int32)
    rows = np.array(sizes, np.int32)
    half = len(sizes) // 2
    totals = [int(rows[:half].sum()), int(rows[half:].sum())]
    ops = T._ops(totals[0]) + T._ops(totals[1], order="rs", flip=False)
    return {"bank": bank, "first": first, "rows": rows, "place": np.array([T._place(rng) for _ in sizes], np.float32),
            "bm_offs": np.array([0, half, len(sizes)], np.int32), "row_offs": np.concatenate([[0], np.cumsum(rows)]).astype(np.int32),
            "ops": np.array(ops, np.float32), "op_offs": np.array([0, len(T._ops(totals[0])), len(ops)], np.int32)}


def _args(t, n_pl, n_out, out_ld, out):
    return (t["bank"].data_ptr(), t["bank"].shape[0], t["first"].data_ptr(), t["rows"].data_ptr(), t["place"].data_ptr(), t["bm_offs"].data_ptr(),
            t["row_offs"].data_ptr(), n_pl, 2, t["ops"].data_ptr(), t["op_offs"].data_ptr(), n_out, out_ld, out)


@pytest.mark.parametrize("out_ld", [3, 4])
@pytest.mark.parametrize("sizes", [(1, 0), (44, 45), (30, 257, 0, 90)], ids=["1", "89", "377"])
def test_place_templates_buffer_contract(sizes, out_ld):
    from btcdet_amd._lib import check, stream_ptr
    host = _case(sizes)
    n_out = int(host["row_offs"][-1])
    want = bc.restate_place_templates(host["bank"], host["first"], host["rows"], host["place"], host["bm_offs"], host["ops"], host["op_offs"], out_ld)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    before = {k: v.clone() for k, v in t.items()}
    out = ac.Guarded((n_out + SPARE, out_ld), "float32")
    ac.call("btc_place_templates", *_args(t, len(sizes), n_out, out_ld, out.ptr))
    assert not bool(out.poison_mask()[:n_out].any()), "a row below n_out was left unwritten"
    assert bool(out.poison_mask()[n_out:].all()), "a row past n_out was written"
    assert out.guards_intact()
    T._same(out.tensor[:n_out].cpu().numpy(), want, ("contract", sizes, out_ld))
    for k, v in before.items():
        assert torch.equal(t[k].reshape(-1).view(torch.uint8), v.reshape(-1).view(torch.uint8)), "input %s was written" % k
    o2 = torch.zeros((n_out + SPARE, out_ld), device="cuda")
    check(L().btc_place_templates(*_args(t, len(sizes), n_out, out_ld, o2.data_ptr()), stream_ptr()), "btc_place_templates")
    torch.cuda.synchronize()
    assert torch.equal(o2[:n_out].view(torch.int32), out.tensor[:n_out].view(torch.int32)) and not bool(o2[n_out:].any())


@pytest.mark.parametrize("garbage", ac.GARBAGE, ids=["a5", "ff"])
def test_garbage_first_and_rows_move_no_write(garbage):
    """bm_first / bm_rows filled with a byte pattern (0xA5A5A5A5 and -1 as int32): rows [0, n_out) are written (zeros where the template
    row they name does not exist), nothing else is, and the bank is not read outside [0, bank_rows)"""
    host = _case((30, 257, 0, 90))
    n_out = int(host["row_offs"][-1])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    for k in ("first", "rows"):
        ac.fill_bytes(t[k], garbage * 0x01010101, 4)
    for out_ld in (3, 4):
        out = ac.Guarded((n_out + SPARE, out_ld), "float32")
        ac.call("btc_place_templates", *_args(t, 4, n_out, out_ld, out.ptr))
        assert not bool(out.poison_mask()[:n_out].any()) and bool(out.poison_mask()[n_out:].all()) and out.guards_intact()
        assert not bool(out.tensor[:n_out, out_ld - 3:].any()), "a negative first or row count names no template row"


def test_nothing_is_written_when_the_arguments_are_refused():
    from btcdet_amd._lib import stream_ptr
    host = _case((30, 257, 0, 90))
    n_out = int(host["row_offs"][-1])
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    out = ac.Guarded((n_out + SPARE, 4), "float32")
    good = list(_args(t, 4, n_out, 4, out.ptr))
    names = ["bank", "bank_rows", "first", "rows", "place", "bm_offs", "row_offs", "n_pl", "batch", "ops", "op_offs", "n_out", "ld", "out"]
    for kw in (dict(ld=2), dict(ld=5), dict(batch=0), dict(n_pl=-1), dict(bank_rows=-1), dict(n_out=-1), dict(n_out=2 ** 31), dict(bm_offs=None),
               dict(row_offs=None), dict(op_offs=None), dict(bank=None), dict(first=None), dict(rows=None), dict(place=None), dict(out=None)):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        assert L().btc_place_templates(*a, stream_ptr()) == -1, kw
    torch.cuda.synchronize()
    assert bool(out.poison_mask().all()) and out.guards_intact()
    a = list(good)
    a[names.index("n_out")], a[names.index("out")] = 0, None          # nothing to do: BTC_OK, nothing launched
    assert L().btc_place_templates(*a, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(out.poison_mask().all())
