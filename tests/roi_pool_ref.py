"""Reference of the ROI head's pooling kernels -- csrc/roi_pool.hip: btc_trilinear_corners / _gather / _scatter -- stage by stage: a
numpy fp32 emulation the GPU has to match BIT FOR BIT, a float64 reference with a derived bound, the shared case lists and the checks
both test modules run (tests/test_roi_pool_ref_cpu.py without a GPU, tests/test_hip_roi_pool_edges.py through the C ABI).  Plain numpy:
no GPU, no autograd.  Conventions of tests/loss_ref.py: a ratio |got - ref| / bound above 1 is a failure, float arguments are
float64(float32(v)), u = 2^-24 (one correctly rounded fp32 operation, relative; the library is built with -ffp-contract=off and the
kernels spell every operation as __f*_rn, so each one rounds on its own).

corners.  Per axis a of (z, y, x), w(a) the world axis (2, 1, 0):
    f = ((p[w] - lo[w]) * (1 / vs[w])) * (1 / stride[a]) - 0.5        range_lo and voxel are (x, y, z), stride_zyx is (z, y, x)
  floor, frac = f - floor, corner c = 4 dz + 2 dy + dx at cell floor + (dz, dy, dx), weight ((z factor) (y factor)) (x factor) with
  factor = frac or 1 - frac, |w|.  A corner is read iff it is inside the grid, its point's scene b = q / points_per_batch is below
  batch and cell_row has a row there; otherwise row -1 and weight 0.  flag = some corner has a row, a NON-ZERO weight and (row_live
  absent or row_live[row]).  `corners_f32` does this with every operation rounded to fp32 on its own: the kernel's bits.
  `corners_f64` is the same geometry in float64.  The fp32 evaluation of f makes at most six roundings (two reciprocals, subtract,
  two multiplies, subtract), each of at most u relative on an intermediate of magnitude at most |f| + 1 (the largest is f + 0.5,
  the reciprocals' errors are relative errors of the products they enter), so to first order
      |f32 - f64| <= delta = 6 u (|f| + 1)                 3.7e-7 (|f| + 1): below 1e-4 for |f| <= 256.
  A point is DECIDED when its three f lie at least MARGIN = 1e-3 from an integer (ten times that delta, so floor agrees), or when it
  lies outside the grid by more than delta on some axis (every corner is outside in both evaluations).  On decided points the rows
  must be equal, the flags must be equal and the weights agree within
      3 delta + 4 u         delta = the largest of the point's three
  : each factor is frac or 1 - frac with frac in [0, 1); frac = f - floor(f) inherits delta and rounds by at most u / 2 (exact by
  Sterbenz for f >= 1, a result in [0.5, 1) otherwise), 1 - frac rounds by at most u / 2 (exact for frac >= 0.5), so a factor is off
  by delta_a + u at most; the factors are at most 1, so the product inherits the sum, 3 delta + 3 u, and its two multiplications
  add u / 2 each (results below 1).  At most CAP = 2 % of a random cloud may be undecided (3 axes x 2 MARGIN = 0.6 % expected).
  On the EXACT geometry (powers of two, quarter-cell lattice) every fp32 operation is exact -- `corners_f64` asserts that every one
  of its own intermediates is an fp32 number -- so every point is decided, integer f included, and the weight bound is 0 + TINY.
gather.  out[p] = t_0 + t_1 + ... + t_7 in corner order, t_c = fp32(feat[row_c] w_c), an absent corner's term +0 (`gather_f32`, the
  kernel's bits).  A term passes through its product and at most seven additions: `gather_f64` bounds by 8 u sum |w f|.
scatter.  grad_feat[row] = sum over the row's segment of w[e] grad_out[e >> 3].  `scatter_emu` walks the kernel's own order: way v
  of WAYS = 256 / C takes the pairs v, v + WAYS, ... of the segment, four at a time into four chains a0..a3 while
  i + 3 WAYS < end, the rest into a0; (a0 + a1) + (a2 + a3); then the ways added in order.  The `any` instance (C not 128 / 64 / 32)
  adds in segment order.  `scatter_f64`: a term passes through its product and at most m additions,
      m = ceil(L / WAYS) + 2 + (WAYS - 1)   (chain, the pair tree, the ways; <= L + WAYS + 2)      m = L for the `any` instance
  so |got - ref| <= (m + 1) u sum |w g| per (row, channel), whatever the order (first order in u; m u < 2e-5 here).

tests/test_roi_pool_ref_cpu.py ties corners_f64 + gather_f64 to conv_head.trilinear_readout and scatter_f64 to torch autograd at
1e-12, runs the emulations over the case lists below and shows for ten seeded defects that some case fails in the defect's stage.
Worst ratio |emulation - float64| / bound per stage over all cases, and the undecided share of the random clouds:

  corners_wts 0.110   gather 0.379   scatter 0.471   (the five bit-exact stages: equal in every case)
  undecided: at most 1.18 % of a cloud (3 points of 255; cap 2 %), worst |f32 - f64| 2.66e-6

The MI355X gives the emulations' bits, hence the same ratios (profiles/roi_pool_edges.txt).
"""
import zlib

import numpy as np

from bn_ref import TINY, ratio, wide

U = 2.0 ** -24
MARGIN = 1e-3
CAP = 0.02
F32 = np.float32

STAGES = ("corners_bits", "corners_rows", "corners_flag", "corners_wts", "gather_bits", "gather", "scatter_bits", "scatter")
EXACT = ("corners_bits", "corners_rows", "corners_flag", "gather_bits", "scatter_bits")
CORNER_DEFECTS = ("stride_zx", "vs_xy", "trunc", "zero_weight_alive", "ignore_live", "corner_dxdydz")
SCATTER_DEFECTS = ("drop_tail", "guard_le", "last_way_omitted", "empty_unwritten")

# lo, vs: (x, y, z); stride: (z, y, x)
GEOMS = {
    "exact": dict(lo=(0.0, 0.0, 0.0), vs=(0.5, 0.25, 1.0), stride=(2.0, 1.0, 4.0), exact=True),
    "kitti": dict(lo=(0.0, -40.0, -3.0), vs=(0.05, 0.05, 0.1), stride=(8.0, 4.0, 2.0), exact=False),
    "skew": dict(lo=(0.1, -0.2, 0.3), vs=(0.3, 0.7, 1.1), stride=(1.0, 2.0, 4.0), exact=False),
}
GRIDS = [("exact", (2, 3, 4), 2), ("exact", (1, 1, 1), 1), ("kitti", (5, 50, 44), 2), ("skew", (3, 7, 9), 2)]
OCCUPANCY = ["full", "empty", "checkerboard", "single"]
LIVE = ["null", "ones", "third_dead", "all_dead"]
Q_LIST = [1, 255, 256, 257, 4096]
PER_BATCH = {1: 7, 255: 128, 256: 128, 257: 100, 4096: 2000}     # 255: a ragged second scene; 257 and 4096: points past batch * per_batch
TRAILING = 5                                                    # the exact lattices' points past batch * points_per_batch
FAR = 1e6

GATHER_C = [1, 16, 63, 64, 65, 130]
GATHER_M = [1, 3, 4, 5]
GATHER_KINDS = ["mixed", "absent", "single"]                    # row p is of kind (p + first) % 3: all eight absent, a single corner
SCATTER_WAYS_C = [128, 64, 32]
SCATTER_ANY_C = [1, 16, 65, 96]
SCATTER_ANY_ROWS = [1, 4, 5]
SCATTER_TAIL = 40                                               # pairs past seg[n_rows]: never read


def scatter_lengths(ways):
    return [0, 1, ways - 1, ways, ways + 1, 4 * ways - 1, 4 * ways, 4 * ways + 1, 8 * ways + 3, 300]


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------------------------ corners
def _cells(cell_row, b, cz, cy, cx, dhw, B):
    """-> row of the cell or -1 (outside the grid, scene past the batch, empty)"""
    D, H, Wd = dhw
    inside = (cz >= 0) & (cz < D) & (cy >= 0) & (cy < H) & (cx >= 0) & (cx < Wd) & (b < B)
    r = cell_row[np.clip(b, 0, B - 1), np.clip(cz, 0, D - 1), np.clip(cy, 0, H - 1), np.clip(cx, 0, Wd - 1)]
    return np.where(inside, r, -1).astype(np.int32)


def _flag(rows, nonzero, row_live, ignore_live=False):
    """some corner has a row, a non-zero weight and, with a row_live table, a live row"""
    live = np.ones(rows.shape, dtype=bool)
    if row_live is not None and not ignore_live:
        table = np.append(np.asarray(row_live, dtype=np.uint8), 0)      # (one entry more: an empty table can be indexed)
        live = table[np.clip(rows, 0, None)] != 0
    return ((rows >= 0) & nonzero & live).any(axis=1).astype(np.uint8)


def _coords_f32(xyz, lo, vs, st):
    """f (Q, 3) in (z, y, x) from float32 operands, one rounding per operation: reciprocal, subtract, multiply, multiply, subtract"""
    one, half = F32(1.0), F32(0.5)
    return np.stack([((xyz[:, w] - lo[w]) * (one / vs[w])) * (one / st[a]) - half for a, w in enumerate((2, 1, 0))], axis=1)


def corners_f32(xyz, per_batch, g, dhw, B, cell_row, row_live, defect=None):
    """the kernel's arithmetic, one fp32 rounding per operation -> rows (Q, 8) int32, weights (Q, 8) float32, flag (Q,) uint8.
    defect: one of CORNER_DEFECTS, a seeded mistake for tests/test_roi_pool_ref_cpu.py"""
    assert defect is None or defect in CORNER_DEFECTS
    xyz = _f32(xyz).reshape(-1, 3)
    Q = xyz.shape[0]
    b = np.arange(Q, dtype=np.int64) // int(per_batch)
    lo, vs, st = [F32(v) for v in g["lo"]], [F32(v) for v in g["vs"]], [F32(v) for v in g["stride"]]
    if defect == "stride_zx":
        st = [st[2], st[1], st[0]]
    if defect == "vs_xy":
        vs = [vs[1], vs[0], vs[2]]
    one = F32(1.0)
    f = _coords_f32(xyz, lo, vs, st)
    fl = np.trunc(f) if defect == "trunc" else np.floor(f)
    fr, lc = list((f - fl).T), list(fl.astype(np.int64).T)
    assert all(x.dtype == np.float32 for x in fr)
    rows, wts = np.empty((Q, 8), np.int32), np.empty((Q, 8), np.float32)
    for c in range(8):
        dz, dy, dx = (c >> 2, (c >> 1) & 1, c & 1) if defect != "corner_dxdydz" else (c & 1, (c >> 1) & 1, c >> 2)
        w = ((fr[0] if dz else one - fr[0]) * (fr[1] if dy else one - fr[1])) * (fr[2] if dx else one - fr[2])
        r = _cells(cell_row, b, lc[0] + dz, lc[1] + dy, lc[2] + dx, dhw, B)
        rows[:, c] = r
        wts[:, c] = np.where(r >= 0, np.abs(w), F32(0.0))
    nonzero = np.ones((Q, 8), dtype=bool) if defect == "zero_weight_alive" else wts != 0
    return rows, wts, _flag(rows, nonzero, row_live, defect == "ignore_live")


def corners_f64(xyz, per_batch, g, dhw, B, cell_row, row_live):
    """float64 -> dict: rows, wts, flag, f (Q, 3) in (z, y, x), decided (Q,), wbound (Q,) = 3 delta + 4 u (TINY on the exact geometry)"""
    xyz = wide(_f32(xyz).reshape(-1, 3))
    Q = xyz.shape[0]
    b = np.arange(Q, dtype=np.int64) // int(per_batch)
    lo, vs, st = [wide(F32(v)) for v in g["lo"]], [wide(F32(v)) for v in g["vs"]], [wide(F32(v)) for v in g["stride"]]
    f = np.empty((Q, 3))
    for a, w in enumerate((2, 1, 0)):
        steps = [xyz[:, w] - lo[w]]
        steps.append(steps[-1] / vs[w])
        steps.append(steps[-1] / st[a])
        steps.append(steps[-1] - 0.5)
        if g["exact"]:   # nothing to round: the reciprocals and every intermediate are fp32 numbers
            for v in [1.0 / vs[w], 1.0 / st[a]] + steps:
                assert np.all(wide(np.asarray(v, dtype=np.float32)) == wide(v)), "the exact geometry is not exact in fp32"
        f[:, a] = steps[-1]
    fl = np.floor(f)
    fr = f - fl
    lc = fl.astype(np.int64)
    rows, wts = np.empty((Q, 8), np.int32), np.empty((Q, 8))
    for c in range(8):
        dz, dy, dx = c >> 2, (c >> 1) & 1, c & 1
        w = (fr[:, 0] if dz else 1.0 - fr[:, 0]) * (fr[:, 1] if dy else 1.0 - fr[:, 1]) * (fr[:, 2] if dx else 1.0 - fr[:, 2])
        r = _cells(cell_row, b, lc[:, 0] + dz, lc[:, 1] + dy, lc[:, 2] + dx, dhw, B)
        rows[:, c] = r
        wts[:, c] = np.where(r >= 0, np.abs(w), 0.0)
    delta = 6.0 * U * (np.abs(f) + 1.0)
    if g["exact"]:
        decided, wbound = np.ones(Q, dtype=bool), np.full(Q, TINY)
    else:
        near = (np.abs(f - np.rint(f)) >= MARGIN).all(axis=1) & (np.abs(f) <= 256.0).all(axis=1)
        dims = wide(dhw)[None, :]
        far = ((f < -1.0 - delta) | (f >= dims + delta)).any(axis=1)
        decided, wbound = near | far, 3.0 * delta.max(axis=1) + 4.0 * U + TINY
    return dict(rows=rows, wts=wts, flag=_flag(rows, wts != 0, row_live), f=f, decided=decided, wbound=wbound)


def coords_f32(xyz, g):
    """the fp32 f alone, (Q, 3) in (z, y, x): what the cap's `worst |f32 - f64|` is measured on"""
    return _coords_f32(_f32(xyz).reshape(-1, 3), *[[F32(v) for v in g[k]] for k in ("lo", "vs", "stride")])


# ------------------------------------------------------------------------------------------------------------------ gather
def gather_f32(feat, rows, wts):
    """the kernel's bits: products rounded, added in corner order, an absent corner contributing +0"""
    feat, wts = _f32(feat), _f32(wts)
    acc = None
    for c in range(8):
        r = rows[:, c]
        with np.errstate(invalid="ignore"):
            t = np.where((r >= 0)[:, None], feat[np.clip(r, 0, None)] * wts[:, c:c + 1], F32(0.0)).astype(np.float32)
        acc = t if acc is None else acc + t
    return acc


def gather_f64(feat, rows, wts):
    """-> (ref (M, C), bound); wts: the table the kernel was given"""
    feat, wts = wide(feat), wide(wts)
    present = rows >= 0
    t = np.where(present[:, :, None], feat[np.clip(rows, 0, None)] * np.where(present, wts, 0.0)[:, :, None], 0.0)
    return t.sum(axis=1), 8.0 * U * np.abs(t).sum(axis=1) + TINY


# ------------------------------------------------------------------------------------------------------------------ scatter
def ways_of(C):
    """WAYS of the instance btc_trilinear_scatter launches for C channels; None: the `any` instance"""
    return 256 // C if C in SCATTER_WAYS_C else None


def scatter_emu(grad_out, pair, seg, wts, n_rows, canary=np.nan, defect=None):
    """the kernel's own summation order -> grad_feat (n_rows, C) float32, every row written over the canary"""
    assert defect is None or defect in SCATTER_DEFECTS
    grad_out, wts = _f32(grad_out), _f32(wts).reshape(-1)
    C = grad_out.shape[1]
    ways = ways_of(C)
    out = np.full((n_rows, C), canary, dtype=np.float32)

    def term(i):
        e = int(pair[i])
        return grad_out[e >> 3] * wts[e]

    with np.errstate(invalid="ignore"):
        for row in range(n_rows):
            s, end = int(seg[row]), int(seg[row + 1])
            if defect == "empty_unwritten" and s == end:
                continue
            if ways is None:
                acc = np.zeros(C, np.float32)
                for i in range(s, end):
                    acc = acc + term(i)
                out[row] = acc
                continue
            part = []
            for way in range(ways):
                a = [np.zeros(C, np.float32) for _ in range(4)]
                i = s + way
                while (i + 3 * ways <= end) if defect == "guard_le" else (i + 3 * ways < end):
                    for k in range(4):
                        a[k] = a[k] + term(i + k * ways)
                    i += 4 * ways
                while i < end and defect != "drop_tail":
                    a[0] = a[0] + term(i)
                    i += ways
                part.append((a[0] + a[1]) + (a[2] + a[3]))
            acc = part[0]
            for way in range(1, ways - (1 if defect == "last_way_omitted" else 0)):
                acc = acc + part[way]
            out[row] = acc
    return out


def scatter_f64(grad_out, pair, seg, wts, n_rows):
    """-> (ref (n_rows, C), bound): (m + 1) u sum |w g|, m the most additions a term passes through"""
    grad_out, wts = wide(grad_out), wide(wts).reshape(-1)
    C = grad_out.shape[1]
    ways = ways_of(C)
    ref, bound = np.zeros((n_rows, C)), np.full((n_rows, C), TINY)
    for row in range(n_rows):
        e = np.asarray(pair[int(seg[row]):int(seg[row + 1])], dtype=np.int64)
        L = e.size
        t = grad_out[e >> 3] * wts[e][:, None]
        m = L if ways is None else -(-L // ways) + 2 + (ways - 1)
        assert m <= L + (ways or 1) + 2
        ref[row] = t.sum(axis=0)
        bound[row] += (m + 1) * U * np.abs(t).sum(axis=0)
    return ref, bound


# ------------------------------------------------------------------------------------------------------------------ case lists
def cell_sizes(g):
    """metres per cell along world (x, y, z)"""
    return [float(F32(g["vs"][w])) * float(F32(g["stride"][a])) for w, a in ((0, 2), (1, 1), (2, 0))]


def lattice(g, dhw):
    """quarter cells from -1.5 to D + 0.5 cells per axis (f from -2 to D: integers, -1, D - 1, fully outside) plus +-FAR: (n, 3) xyz"""
    cs = cell_sizes(g)
    ax = [np.float64(g["lo"][w]) + (np.arange(-6, 4 * n + 3) / 4.0) * cs[w] for w, n in ((0, dhw[2]), (1, dhw[1]), (2, dhw[0]))]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    pts = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)
    return np.concatenate([pts, [[FAR, FAR, FAR], [-FAR, 0.25, -FAR]]]).astype(np.float32)


def corner_cases(grids=None):
    out = []
    for (gname, dhw, B) in (GRIDS if grids is None else grids):
        for occ in OCCUPANCY:
            for live in LIVE:
                for Q in ([None] if GEOMS[gname]["exact"] else Q_LIST):
                    out.append(dict(geom=gname, dhw=dhw, B=B, occ=occ, live=live, Q=Q))
    return out


def case_name(c):
    return "-".join("x".join(str(i) for i in v) if isinstance(v, tuple) else str(v) for v in c.values())


def make_corners(c):
    """-> dict xyz, per_batch, g, dhw, B, cell_row, n_rows, row_live (None: NULL), random (a cloud the cap applies to)"""
    g, dhw, B = GEOMS[c["geom"]], c["dhw"], c["B"]
    rng = np.random.default_rng(_seed("corners", c["geom"], dhw, B, c["occ"], c["Q"]))
    D, H, Wd = dhw
    if g["exact"]:
        lat = lattice(g, dhw)
        per_batch = lat.shape[0]
        inside = lat[(np.abs(lat) < 1e5).all(axis=1)]
        xyz = np.concatenate([lat] * B + [inside[:: max(inside.shape[0] // TRAILING, 1)][:TRAILING]])
    else:
        Q, per_batch = c["Q"], PER_BATCH[c["Q"]]
        cs, lo = cell_sizes(g), [float(F32(v)) for v in g["lo"]]
        t = np.stack([rng.uniform(-1.5, n + 0.5, Q) for n in (Wd, H, D)], axis=1)
        xyz = (np.array(lo) + t * np.array(cs)).astype(np.float32)
        if Q >= 255:
            xyz[7], xyz[Q - 1] = [FAR, -FAR, FAR], [-FAR, FAR, 1.0]
    b, z, y, x = np.meshgrid(np.arange(B), np.arange(D), np.arange(H), np.arange(Wd), indexing="ij")
    if c["occ"] == "full":
        present = np.ones((B, D, H, Wd), dtype=bool)
    elif c["occ"] == "empty":
        present = np.zeros((B, D, H, Wd), dtype=bool)
    elif c["occ"] == "checkerboard":
        present = (b + z + y + x) % 2 == 0
    else:
        present = (b == B - 1) & (z == D // 2) & (y == H // 2) & (x == Wd // 2)
    n_rows = int(present.sum())
    cell_row = np.full((B, D, H, Wd), -1, dtype=np.int32)
    cell_row[present] = rng.permutation(n_rows).astype(np.int32)      # a row number says nothing about where its cell lies
    live = {"null": None, "ones": np.ones(n_rows, np.uint8), "third_dead": (np.arange(n_rows) % 3 != 0).astype(np.uint8),
            "all_dead": np.zeros(n_rows, np.uint8)}[c["live"]]
    return dict(xyz=xyz, per_batch=per_batch, g=g, dhw=dhw, B=B, cell_row=cell_row, n_rows=n_rows, row_live=live,
                random=not g["exact"] and c["Q"] >= 255)


def gather_cases():
    return [dict(C=C, M=M, first=k) for C in GATHER_C for M in GATHER_M for k in range(3)]


def make_gather(c, n_feat=7):
    """-> feat (n_feat, C), rows (M, 8), wts (M, 8): NaN where the corner is absent (the kernel must not use it)"""
    rng = np.random.default_rng(_seed("gather", *c.values()))
    C, M = c["C"], c["M"]
    feat = rng.standard_normal((n_feat, C)).astype(np.float32)
    rows = rng.integers(-1, n_feat, (M, 8)).astype(np.int32)
    for p in range(M):
        kind = GATHER_KINDS[(p + c["first"]) % 3]
        if kind == "absent":
            rows[p] = -1
        elif kind == "single":
            keep = int(rng.integers(0, 8))
            rows[p, np.arange(8) != keep] = -1
            rows[p, keep] = int(rng.integers(0, n_feat))
    wts = rng.uniform(0.0, 1.0, (M, 8)).astype(np.float32)
    wts[rows < 0] = np.nan
    return dict(feat=feat, rows=rows, wts=wts)


def scatter_cases():
    out = [dict(C=C, lengths=scatter_lengths(256 // C)) for C in SCATTER_WAYS_C]
    base = [0, 3, 1, 17, 5]
    for k, C in enumerate(SCATTER_ANY_C):
        for n in SCATTER_ANY_ROWS:
            out.append(dict(C=C, lengths=(base[k:] + base[:k])[:n]))
    return out


def scatter_name(c):
    return f"C{c['C']}-" + "_".join(str(v) for v in c["lengths"])


def make_scatter(c):
    """synthetic pair lists -> grad_out (P, C), pair, seg, wts (P, 8), n_rows.  Every (point, corner) slot that no segment holds --
    the SCATTER_TAIL pairs behind seg[n_rows] among them -- has a NaN weight: reading one shows in the result"""
    rng = np.random.default_rng(_seed("scatter", c["C"], *c["lengths"]))
    C, lengths = c["C"], list(c["lengths"])
    total = sum(lengths) + SCATTER_TAIL
    P = -(-total // 8) + 3
    slots = rng.permutation(P * 8)[:total]
    pair, seg, at = [], [0], 0
    for L in lengths:
        pair.append(np.sort(slots[at:at + L]))         # in pair order inside a row, as the stable sort leaves them
        at += L
        seg.append(at)
    pair.append(slots[at:])
    pair = np.concatenate(pair).astype(np.int32)
    wts = np.full(P * 8, np.nan, dtype=np.float32)
    wts[pair[:seg[-1]]] = rng.uniform(0.05, 1.0, seg[-1]).astype(np.float32)
    grad_out = rng.standard_normal((P, C)).astype(np.float32)
    return dict(grad_out=grad_out, pair=pair, seg=np.array(seg, np.int32), wts=wts.reshape(P, 8), n_rows=len(lengths))


# ------------------------------------------------------------------------------------------------------------------ the checks
class Worst:
    """worst ratio per stage over everything checked through it; strict: a ratio above 1 raises"""

    def __init__(self, strict=True):
        self.worst, self.strict = {}, strict
        self.undecided, self.coord_err = 0.0, 0.0

    def check(self, stage, got, ref_bound, where=""):
        assert stage in STAGES and stage not in EXACT, stage
        return self._note(stage, ratio(got, *ref_bound), where)

    def exact(self, stage, got, ref, where=""):
        """bit-exact stages: ratio 0 or inf"""
        assert stage in EXACT, stage
        return self._note(stage, 0.0 if bits_equal(got, ref) else np.inf, where)

    def _note(self, stage, r, where):
        self.worst[stage] = max(self.worst.get(stage, 0.0), r)
        if self.strict:
            assert r <= 1.0, f"{stage} {where}: |got - ref| is {r:.3g} of its bound"
        return r

    def require(self, cond, where=""):
        if self.strict:
            assert cond, where
        elif not cond:
            self.worst["require"] = np.inf

    def report(self):
        return "worst |got - ref| / bound: " + "  ".join(f"{s} {self.worst[s]:.3f}" for s in STAGES if s in self.worst) \
            + f"   undecided: at most {100 * self.undecided:.2f} % of a cloud, worst |f32 - f64| {self.coord_err:.3g}"


def check_corners(W, d, rows, wts, flag, where=""):
    """the corner stage's outputs (numpy: int32, float32, uint8) for make_corners' inputs d"""
    e_rows, e_wts, e_flag = corners_f32(d["xyz"], d["per_batch"], d["g"], d["dhw"], d["B"], d["cell_row"], d["row_live"])
    W.exact("corners_bits", rows, e_rows, where + " rows")
    W.exact("corners_bits", wts, e_wts, where + " weights")
    W.exact("corners_bits", flag, e_flag, where + " flag")
    r = corners_f64(d["xyz"], d["per_batch"], d["g"], d["dhw"], d["B"], d["cell_row"], d["row_live"])
    ok = r["decided"]
    if d["random"]:
        share = 1.0 - float(ok.mean())
        W.undecided = max(W.undecided, share)
        W.require(share <= CAP, f"{where}: {100 * share:.2f} % of the cloud undecided")
        near = (np.abs(r["f"]) <= 256.0).all(axis=1)
        err = np.abs(wide(coords_f32(d["xyz"], d["g"])) - r["f"])[near]
        W.coord_err = max(W.coord_err, float(err.max()) if err.size else 0.0)
        W.require(bool((err <= (6.0 * U * (np.abs(r["f"]) + 1.0))[near]).all()), f"{where}: |f32 - f64| above 6 u (|f| + 1)")
    else:
        W.require(bool(ok.all()) or not d["g"]["exact"], f"{where}: an undecided point on the exact geometry")
    if rows.shape == r["rows"].shape and flag.shape == r["flag"].shape:
        W.exact("corners_rows", rows[ok], r["rows"][ok], where)
        W.exact("corners_flag", flag[ok], r["flag"][ok], where)
        W.check("corners_wts", wts[ok], (r["wts"][ok], np.repeat(r["wbound"][ok][:, None], 8, axis=1)), where)
    past = np.arange(rows.shape[0]) >= d["B"] * d["per_batch"]
    W.require(bool((rows[past] == -1).all() and (wts[past] == 0).all() and (flag[past] == 0).all()),
              f"{where}: a point past batch * points_per_batch read something")


def check_gather(W, d, out, where=""):
    W.exact("gather_bits", out, gather_f32(d["feat"], d["rows"], d["wts"]), where)
    W.check("gather", out, gather_f64(d["feat"], d["rows"], d["wts"]), where)


def check_scatter(W, d, grad_feat, where=""):
    W.exact("scatter_bits", grad_feat, scatter_emu(d["grad_out"], d["pair"], d["seg"], d["wts"], d["n_rows"]), where)
    W.check("scatter", grad_feat, scatter_f64(d["grad_out"], d["pair"], d["seg"], d["wts"], d["n_rows"]), where)
