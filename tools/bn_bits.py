"""The bits of the BatchNorm family of csrc/bn.hip, case by case: one line per case with the sha256 (first 16 hex digits) of every output of one forward +
backward + column sum (mean, rstd, y, running_mean, running_var, nbt, dx, dgamma, dbeta, col_sum; `-` where the mode has none).  Run it
in two builds and diff the outputs: the fp64 additions of these kernels are written in a fixed order, so a refactor changes no bit.

Cases, all from tests/test_hip_bn_edges.py: CHANNELS x row_counts(C) x MODES in fp32, BF16_CHANNELS x row_counts(C) in bf16, the
test_grid_edges list, WS_SHAPES with tuning keys 9 and 10 at 0, 1 and 4096.  Inputs: tests/bn_ref.py make_inputs with fixed seeds."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import bn_ref as R
import test_hip_bn_edges as T
from btcdet_amd._lib import check, lib

KEYS = ["mean", "rstd", "y", "running_mean", "running_var", "nbt", "dx", "dgamma", "dbeta", "col_sum"]
GRID_EDGES = [(511, 32), (512, 32), (513, 32), (341, 32), (342, 32), (131073, 32), (526337, 5)]   # test_grid_edges


def case(what, n, c, seed, mode="train_running", bf16=False):
    """run_case of the test module without its checks, through the C ABI on a workspace of its own"""
    training, running = mode != "eval", mode != "train_null"
    d = R.make_inputs(n, c, seed, bf16)
    tdt = torch.bfloat16 if bf16 else torch.float32
    x, dy, g, b = T.up(d["x"], tdt), T.up(d["dy"], tdt), T.up(d["gamma"]), T.up(d["beta"])
    rm, rv = (T.up(d["running_mean"]), T.up(d["running_var"])) if running else (None, None)
    nbt = torch.full((), 5, dtype=torch.long, device=T.dev()) if (running and training) else None
    api = T.Abi(T._ws(lib().btc_bn_ws_bytes(c)))
    y, stats = api.fwd(x, g, b, rm, rv, nbt, training, True)
    dx, dg, db = api.bwd(x, y, dy, g, stats, training, True)
    o = dict(mean=stats[0], rstd=stats[1], y=y, running_mean=rm, running_var=rv, nbt=nbt, dx=dx, dgamma=dg, dbeta=db, col_sum=api.col_sum(x))
    torch.cuda.synchronize()
    sha = lambda t: "-" if t is None else hashlib.sha256(t.reshape(-1).contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]
    print("%-44s %s" % (what, " ".join(sha(o[k]) for k in KEYS)), flush=True)


print("%-44s %s" % ("# case", " ".join(KEYS)))
for C in T.CHANNELS:
    for n in T.row_counts(C):
        for mode in T.MODES:
            case("fp32 N %d C %d %s" % (n, C, mode), n, C, 1000 * C + n, mode)
for C in T.BF16_CHANNELS:
    for n in T.row_counts(C):
        case("bf16 N %d C %d" % (n, C), n, C, 1000 * C + n + 500000, bf16=True)
for n, c in GRID_EDGES:
    case("grid N %d C %d" % (n, c), n, c, n + c)
for c, n in T.WS_SHAPES.items():
    for key in (9, 10):
        for value in (0, 1, 4096):
            check(lib().btc_tune_set(key, value), "btc_tune_set")
            try:
                case("tuned N %d C %d key %d = %d" % (n, c, key, value), n, c, 10 * key + value + c)
            finally:
                check(lib().btc_tune_set(key, 0), "btc_tune_set")
