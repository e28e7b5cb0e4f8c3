"""Greedy-NMS scenes with a kept list known by construction, and an independent float64 reference (plain numpy, no device code).

The three greedy chains of the library (nms_reduce and topk_chain of csrc/iou3d_nms.hip, step 5 of det_select_nms of csrc/det_post.hip)
decide from a bit mask, 64 boxes to a word.  A random scene cannot put a suppressor and its victim on a chosen lane, word or chunk;
these scenes can.  A scene is n boxes in SORTED order (descending score: position 0 is the best box) built from sites:

* sites lie on a square grid of 16 m pitch centred on the origin; site k has heading HEADINGS[k % 10]; sites are numbered in the
  order in which the sorted positions first reach them;
* every box is 4 x 2 x 1.5 m and sits at its site's centre, shifted along the site's heading by 0, 1.5 or 3 m;
* boxes of different sites are at least 16 - 2 * 3 = 10 m apart, more than two half-diagonals (2 * 2.24 m) + 1 m: they never overlap;
* two boxes of one site whose shifts differ by d overlap in a (4 - d) x 2 rectangle:
      d = 0: IoU 1        d = 1.5: IoU 5 / 11 = 0.4545        d = 3: IoU 2 / 14 = 0.1429
  so with the threshold THRESH = 0.3 a kept box suppresses the later boxes of its site whose shift differs by at most 1.5 m, and
  every IoU of a scene lies at least MARGIN = 0.1 from the threshold (build() asserts it on float64 IoUs): no fp32 formulation of the
  overlap can flip a decision, so the tests compare kept lists for equality, with no escape clause.

For the axis-aligned chains (rotated=False) the geometry uses heading 0 and column 6 holds arbitrary non-zero headings, which the
chain has to ignore.

Primitives, each on a site of its own, addressed by sorted positions (every other position is a singleton on its own site):

    pair(p, q), p < q       shifts 0, 1.5: q is suppressed
    triple(a, b, c)         shifts 0, 1.5, 3 with a < b and a < c: b is suppressed by a, and c is KEPT -- IoU(a, c) is below the
                            threshold, and b, itself suppressed, suppresses nothing (a < b < c); with a < c < b, b falls to a
    pile(p0, p1, ...)       identical boxes: only the first survives

reference_keep() is the float64 greedy loop the expectation is pinned against (tests/test_nms_scenes_cpu.py): the Sutherland-Hodgman
clipper of tests/test_oracle_iou3d.py for rotated boxes, the closed form for axis-aligned ones, evaluated for the pairs whose centres
are closer than the sum of their half-diagonals + 1 m only (every other pair is 0 by geometry: 16 000-box scenes stay cheap)."""
import functools
from collections import namedtuple

import numpy as np

from test_oracle_iou3d import _clip_area, _corners

THRESH = 0.3
MARGIN = 0.1
PITCH = 16.0
DIMS = (4.0, 2.0, 1.5)
HEADINGS = [0.0, np.pi / 2, np.pi, -np.pi, np.pi / 4, 0.3, -2.1, 1e-3, np.pi / 2 - 1e-3, 3 * np.pi / 4]
NONFINITE_KINDS = ("nan_centre", "inf_length", "nan_heading", "all_zero")

Scene = namedtuple("Scene", ["boxes", "keep", "n", "rotated", "ious", "pairs", "triples", "piles"])


# ------------------------------------------------------------------------------------------------------------ float64 reference
def iou_f64(a, b, rotated):
    """exact BEV IoU of two float64 box rows"""
    if rotated:
        inter = _clip_area(_corners(a), _corners(b))
    else:
        w = min(a[0] + a[3] / 2, b[0] + b[3] / 2) - max(a[0] - a[3] / 2, b[0] - b[3] / 2)
        h = min(a[1] + a[4] / 2, b[1] + b[4] / 2) - max(a[1] - a[4] / 2, b[1] - b[4] / 2)
        inter = max(w, 0.0) * max(h, 0.0)
    return inter / max(a[3] * a[4] + b[3] * b[4] - inter, 1e-12)


def pair_ious(boxes, rotated):
    """{(i, j), i < j: float64 IoU} over the pairs whose centres are closer than their half-diagonals + 1 m (all others: 0)"""
    b = np.asarray(boxes, dtype=np.float64)
    n = b.shape[0]
    if n == 0:
        return {}
    rad = 0.5 * np.hypot(b[:, 3], b[:, 4])
    cell = 2 * float(rad.max()) + 1.0
    cx, cy = np.floor(b[:, 0] / cell).astype(np.int64).tolist(), np.floor(b[:, 1] / cell).astype(np.int64).tolist()
    buckets = {}
    for i in range(n):
        buckets.setdefault((cx[i], cy[i]), []).append(i)
    out = {}
    for (kx, ky), members in buckets.items():
        near = [j for dx in (-1, 0, 1) for dy in (-1, 0, 1) for j in buckets.get((kx + dx, ky + dy), ())]
        if len(near) == 1:
            continue
        for i in members:
            for j in near:
                if j > i and np.hypot(b[i, 0] - b[j, 0], b[i, 1] - b[j, 1]) < rad[i] + rad[j] + 1.0:
                    out[(i, j)] = iou_f64(b[i], b[j], rotated)
    return out


def reference_keep(boxes, rotated, thresh=THRESH, ious=None):
    """plain greedy NMS over boxes in sorted order with float64 IoUs -> kept positions, ascending"""
    n = len(boxes)
    if ious is None:
        ious = pair_ious(boxes, rotated)
    later = {}
    for (i, j), v in ious.items():
        if v > thresh:
            later.setdefault(i, []).append(j)
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        for j in later.get(i, ()):
            removed[j] = True
    return np.asarray(keep, np.int64)


# ------------------------------------------------------------------------------------------------------------------ the builder
def nonfinite_row(kind, like):
    row = np.array(like, np.float32)
    if kind == "nan_centre":
        row[0] = np.nan
    elif kind == "inf_length":
        row[3] = np.inf
    elif kind == "nan_heading":
        row[6] = np.nan
    elif kind == "all_zero":
        row[:] = 0
    else:
        raise ValueError(kind)
    return row


def build(n, pairs=(), triples=(), piles=(), rotated=True, removed=(), nonfinite=None):
    """-> Scene.  removed: positions that are no candidates (the fused chain's score threshold): they are neither kept nor
    suppress; nonfinite: {singleton position: kind of NONFINITE_KINDS}, rows overwritten AFTER the margin check (such a row overlaps
    nothing, so it stays what its position was: a kept singleton)."""
    prims = []   # (positions, shifts)
    for p, q in pairs:
        assert p < q, (p, q)
        prims.append(((p, q), (0.0, 1.5)))
    for a, b, c in triples:
        assert a < b and a < c, (a, b, c)
        prims.append(((a, b, c), (0.0, 1.5, 3.0)))
    for pile in piles:
        assert len(pile) >= 2 and list(pile) == sorted(pile), pile
        prims.append((tuple(pile), (0.0,) * len(pile)))
    prim_of = np.full(n, -1, np.int64)
    shift = np.zeros(n, np.float64)
    for k, (pos, sh) in enumerate(prims):
        for p, s in zip(pos, sh):
            assert 0 <= p < n and prim_of[p] < 0, "position %d outside the scene or in two primitives" % p
            prim_of[p] = k
            shift[p] = s
    # sites in the order in which the positions reach them
    site = np.zeros(n, np.int64)
    prim_site = {}
    nsites = 0
    for p in range(n):
        k = int(prim_of[p])
        if k < 0 or k not in prim_site:
            if k >= 0:
                prim_site[k] = nsites
            site[p] = nsites
            nsites += 1
        else:
            site[p] = prim_site[k]
    G = max(int(np.ceil(np.sqrt(max(nsites, 1)))), 1)
    sx = (site % G - (G - 1) / 2.0) * PITCH
    sy = (site // G - (G - 1) / 2.0) * PITCH
    head = np.asarray(HEADINGS, np.float64)[site % len(HEADINGS)] if rotated else np.zeros(n)
    boxes = np.zeros((n, 7), np.float32)
    boxes[:, 0] = sx + shift * np.cos(head)
    boxes[:, 1] = sy + shift * np.sin(head)
    boxes[:, 2] = (np.arange(n) % 5) * 0.1 - 0.2
    boxes[:, 3:6] = DIMS
    boxes[:, 6] = head if rotated else 0.5 + 0.37 * (np.arange(n) % 11)   # axis-aligned chains must ignore column 6
    # the expectation, by construction: within a primitive, in position order, a kept member suppresses shifts within 1.5 m
    gone = np.zeros(n, bool)
    gone[list(removed)] = True
    for pos, sh in prims:
        members = sorted(zip(pos, sh))
        kept = []
        for p, s in members:
            if gone[p]:
                continue
            if any(abs(s - t) <= 1.5 for t in kept):
                gone[p] = True
            else:
                kept.append(s)
    keep = np.flatnonzero(~gone).astype(np.int64)
    # the condition: every pair's exact IoU at least MARGIN from the threshold (pairs not listed are 0 by geometry)
    ious = pair_ious(boxes, rotated)
    for ij, v in ious.items():
        assert abs(v - THRESH) >= MARGIN, "IoU %.4f of positions %s is within %.2f of the threshold" % (v, ij, MARGIN)
    if nonfinite:
        for p, kind in nonfinite.items():
            assert prim_of[p] < 0, "non-finite rows replace singletons"
            boxes[p] = nonfinite_row(kind, boxes[p])
    return Scene(boxes, keep, n, rotated, ious, tuple(pairs), tuple(triples), tuple(tuple(p) for p in piles))


def clip_prims(n, pairs, triples):
    """the primitives that fit n positions: a triple whose c falls outside stays as the pair (a, b)"""
    ps = [(p, q) for p, q in pairs if q < n]
    ts = []
    for a, b, c in triples:
        if max(a, b, c) < n:
            ts.append((a, b, c))
        elif a < n and b < n:
            ps.append((a, b))
    return ps, ts


def filler_pairs(lo, hi, used):
    """adjacent pairs (p, p + 1) over the free positions of [lo, hi): every second box of the range is suppressed"""
    used = set(used)
    out, p = [], lo
    while p + 1 < hi:
        if p in used or p + 1 in used:
            p += 1
            continue
        out.append((p, p + 1))
        p += 2
    return out


def pile_fill(lo, hi, count):
    """[lo, hi) cut into `count` contiguous piles of near-equal size (each of at least 2 boxes): exactly `count` boxes survive"""
    assert count >= 1 and hi - lo >= 2 * count, (lo, hi, count)
    edges = np.linspace(lo, hi, count + 1).round().astype(int)
    return [tuple(range(edges[k], edges[k + 1])) for k in range(count)]


def _used(pairs, triples):
    return {p for t in list(pairs) + list(triples) for p in t}


def rank_of(scene, pos):
    """kept rank of a kept position"""
    r = int(np.searchsorted(scene.keep, pos))
    assert r < len(scene.keep) and scene.keep[r] == pos, "position %d is not kept" % pos
    return r


# ------------------------------------------------------------------------------------------------- the catalogue: the full chain
# victim lanes 1, 31, 32, 63 of the suppressor's own word (words 0 and 1); lanes 0, 31, 32, 63 of the next word (word 2 -> 3) and of
# the word four further on (word 1 -> 5, word 2 -> 6); suppressors on lanes 0 (positions 0, 64, 128), 31 (95, 159) and 63 (191)
WORD_EDGE_PAIRS = ((0, 1), (2, 31), (3, 32), (4, 63), (95, 96), (65, 127),
                   (128, 192), (159, 223), (191, 224), (129, 255),
                   (64, 320), (97, 351), (98, 352), (126, 383),
                   (160, 384), (190, 415), (130, 416), (131, 447))
WORD_EDGE_N = 448
# inside one word; a, b in word 1 and c in word 2; three different words; a < c < b inside word 2; a < c < b over three words
TRIPLES = ((10, 20, 30), (70, 100, 130), (5, 80, 200), (140, 190, 150), (40, 250, 110))
TRIPLES_N = 256
SMALL_N = (1, 2, 63, 64, 65, 128, 129)
LONG_N = 16500   # 258 words: word 257 is the second trip of nms_reduce's `j += 256` loop from word 0, and partial (52 boxes)
# suppressors in word 0 (and one in word 1); victims on lanes 0 / 63 of word 255, 0 / 31 / 32 / 63 of word 256, 0 / 31 / 32 / 51 (the
# last box) of word 257
LONG_PAIRS = ((0, 16320), (1, 16383), (2, 16384), (31, 16415), (32, 16416), (63, 16447), (3, 16448), (5, 16479), (6, 16480),
              (7, 16499), (64, 16449))
LONG_TRIPLES = ((8, 40, 16460), (9, 16450, 16490))   # c in word 257; b and c both in word 257


@functools.lru_cache(maxsize=None)
def small(n, rotated, with_pair):
    return build(n, pairs=[(0, n - 1)] if (with_pair and n >= 2) else [], rotated=rotated)


@functools.lru_cache(maxsize=None)
def word_edges(rotated, n=WORD_EDGE_N):
    """n > 448: singletons after the seven words (a batch mate for the top-k scenes of 832 and 900 boxes)"""
    return build(n, pairs=WORD_EDGE_PAIRS, rotated=rotated)


@functools.lru_cache(maxsize=None)
def triples(rotated):
    return build(TRIPLES_N, triples=TRIPLES, rotated=rotated)


@functools.lru_cache(maxsize=None)
def piles(rotated):
    """word 9 (576 .. 639) wholly suppressed from position 7 of word 0: a word whose kept mask is empty, followed by word 10 with a
    victim (650) and singletons; a pile strided over lane 9 of words 0 .. 7"""
    return build(704, pairs=[(10, 650)], piles=[(7,) + tuple(range(576, 640)), tuple(9 + 64 * k for k in range(8))], rotated=rotated)


@functools.lru_cache(maxsize=None)
def long_scene(rotated):
    return build(LONG_N, pairs=LONG_PAIRS, triples=LONG_TRIPLES, rotated=rotated)


# ---------------------------------------------------------------------------------------------- the catalogue: the top-k chain
# btc_nms_topk takes the candidates in chunks [0, 768), [768, 2304), [2304, 4864), [4864, ...); a box kept in a chunk is copied to kept
# slot `rank` of K = max_keep rounded up to 64 slots, from where it suppresses the candidates of the later chunks.
CHUNK_N = (769, 2305, 4865, 5000)
CHUNK_MAX_KEEP = 4096
# variant 0: suppressors of kept ranks 0, 63, 64 (and 62, 65) in chunk 0, victims at the chunk edges 768, 2303, 2304, 4863, 4864
# variant 1: the triples (13, 2303, 2304) and (767, 768, 4864): b on one side of a chunk edge, c on the other, a in a kept slot
CHUNK_PRIMS = (
    (((0, 768), (63, 2303), (64, 2304), (62, 4863), (65, 4864)), ((10, 800, 2400),)),
    (((0, 4863), (63, 769), (64, 2305)), ((13, 2303, 2304), (767, 768, 4864))),
)


@functools.lru_cache(maxsize=None)
def chunk_edges(n, variant, rotated):
    """never fills max_keep = 4096: above 4096 boxes, adjacent filler pairs in [1000, 2300) and [2500, 4800) halve the kept count"""
    ps, ts = clip_prims(n, *CHUNK_PRIMS[variant])
    if n > CHUNK_MAX_KEEP:
        used = _used(ps, ts)
        ps = ps + filler_pairs(1000, 2300, used) + filler_pairs(2500, 4800, used)
    sc = build(n, pairs=ps, triples=ts, rotated=rotated)
    assert len(sc.keep) < CHUNK_MAX_KEEP
    for p in (0, 62, 63, 64, 65):
        assert rank_of(sc, p) == p      # the suppressors' kept slots: lanes 0, 62, 63 of slot word 0; lanes 0, 1 of slot word 1
    return sc


LAST_SLOT_MAX_KEEP = 704   # K = 704: 11 slot words


@functools.lru_cache(maxsize=None)
def last_slot(variant, rotated):
    """n = 769, max_keep = K = 704.  Variants 0 and 1: 65 victims in chunk 0, so position 767 holds kept rank 702 = K - 2, lane 62 of the
    LAST slot word, and suppresses 768, the first box of chunk 1; 703 boxes are kept, the scene never fills.  (Rank K - 1 cannot
    suppress across a chunk edge: keeping it fills the scene and ends the chain.)  Variant 2: 64 victims, 767 holds rank K - 1 = 703
    and fills the scene with the last box of chunk 0."""
    lo = (100, 300, 100)[variant]
    cnt = (65, 65, 64)[variant]
    sc = build(769, pairs=[(lo + 2 * i, lo + 2 * i + 1) for i in range(cnt)] + [(767, 768)], rotated=rotated)
    assert rank_of(sc, 767) == (702, 702, 703)[variant] and len(sc.keep) == (703, 703, 704)[variant]
    return sc


CAPS = (1, 63, 64, 65, 100, 256)
CAP_N = 832
CAP_KINDS = ("mid", "at767", "at768", "never")


def cap_kinds(max_keep):
    return CAP_KINDS if max_keep >= 2 else ("mid",)     # with max_keep = 1 the only kept box is position 0


@functools.lru_cache(maxsize=None)
def cap(max_keep, kind, rotated):
    """n = 832.  mid: ten adjacent pairs in [0, 20), then singletons: the max_keep-th kept box sits at max_keep + 9, inside a word, with
    keepable boxes after it in that word.  at767 / at768: max_keep - 1 piles over [0, 767) / [0, 768), singletons after them: the
    max_keep-th kept box is the last box of chunk 0 / the first of chunk 1.  never: max_keep - 1 piles over the whole scene."""
    M = max_keep
    if kind == "mid":
        sc = build(CAP_N, pairs=[(2 * i, 2 * i + 1) for i in range(10)], rotated=rotated)
        assert sc.keep[M - 1] == (M + 9 if M > 10 else 2 * (M - 1)) and len(sc.keep) > M
    elif kind in ("at767", "at768"):
        edge = 767 if kind == "at767" else 768
        sc = build(CAP_N, piles=pile_fill(0, edge, M - 1), rotated=rotated)
        assert sc.keep[M - 1] == edge and len(sc.keep) > M
    else:
        sc = build(CAP_N, piles=pile_fill(0, CAP_N, M - 1), rotated=rotated)
        assert len(sc.keep) == M - 1
    return sc


FILL_N, FILL_MAX_KEEP = 5000, 4096


@functools.lru_cache(maxsize=None)
def fill4096(variant, rotated):
    """max_keep = K = 4096, n = 5000: 800 filler victims, so the kept slots fill over all four chunks and the 4096th kept box sits in
    chunk 3, near position 4900, with keepable boxes after it.  The pairs' suppressors hold kept ranks in the last slot word
    (4032 .. 4094): one pair inside chunk 2 (victim 4863, its last box), one across the edge 4864, one inside chunk 3."""
    lo = (1000, 900)[variant]
    d = (0, 3)[variant]
    ps = [(4835 + d, 4863), (4840 + d, 4870 + d), (4866 + d, 4880 + d)]
    ps = ps + filler_pairs(lo, lo + 1600, _used(ps, ()))
    sc = build(FILL_N, pairs=ps, rotated=rotated)
    for p, _ in ps[:3]:
        assert 4032 <= rank_of(sc, p) <= 4094
    assert len(sc.keep) > FILL_MAX_KEEP and 4864 < sc.keep[FILL_MAX_KEEP - 1] < FILL_N - 64
    return sc


THREE_N, THREE_MAX_KEEP = 2500, 704


@functools.lru_cache(maxsize=None)
def three(which, rotated):
    """one batch, max_keep = 704: scene 0 fills in chunk 0 (singletons and a few pairs), scene 1 in chunk 2 (700 piles over
    [0, 2304), singletons after them), scene 2 never (650 piles over the whole scene)"""
    if which == 0:
        sc = build(THREE_N, pairs=[(3, 9), (64, 127), (700, 701)], rotated=rotated)
        assert sc.keep[THREE_MAX_KEEP - 1] < 768
    elif which == 1:
        sc = build(THREE_N, piles=pile_fill(0, 2304, 700), rotated=rotated)
        assert sc.keep[THREE_MAX_KEEP - 1] == 2307
    else:
        sc = build(THREE_N, piles=pile_fill(0, THREE_N, 650), rotated=rotated)
        assert len(sc.keep) == 650
    return sc


# ---------------------------------------------------------------------------------------------- the catalogue: the fused chain
FUSED_M = (1024, 1000)
FUSED_TRIPLES = tuple(tuple(448 + p for p in t) for t in TRIPLES)   # 448 = 7 words: the triples keep their lanes
FUSED_REMOVED = (0, 128, 458, 588)   # suppressors of the pairs (0, 1) and (128, 192), a of the triples (458, 468, 478), (588, 638, 598)


def fused_prims(m):
    # ... and a victim on the last candidate, one on lane 0 of the last word, one pair astride pre_max = 700
    return WORD_EDGE_PAIRS + ((700, m - 1), (701, 960), (450, 702)), FUSED_TRIPLES


@functools.lru_cache(maxsize=None)
def fused(m, rotated, removed=False):
    """removed: the positions FUSED_REMOVED fall below the score threshold: 1 and 192 are kept; b = 468 is kept and suppresses c = 478;
    of (588, 638, 598), a < c < b, c = 598 is kept and suppresses b = 638 in a's place"""
    ps, ts = fused_prims(m)
    sc = build(m, pairs=ps, triples=ts, rotated=rotated, removed=FUSED_REMOVED if removed else ())
    if removed:
        kept = set(sc.keep.tolist())
        assert {1, 192, 468, 598} <= kept and not ({478, 638} | set(FUSED_REMOVED)) & kept
    return sc


# ------------------------------------------------------------------------------------------------------------- non-finite rows
NONFINITE_PAIRS = ((0, 1), (10, 70), (63, 64), (100, 199), (6, 800), (68, 769))
NONFINITE_TRIPLES = ((20, 30, 40),)
NONFINITE_AT = (5, 66, 67, 130, 770, 771, 772, 773)     # kinds in the order of NONFINITE_KINDS, twice


@functools.lru_cache(maxsize=None)
def nonfinite(n, rotated):
    """n = 200 (one chunk, four words) or 900 (the rows 770 .. 773 enter the top-k chain's kept slots in chunk 1)"""
    ps, ts = clip_prims(n, NONFINITE_PAIRS, NONFINITE_TRIPLES)
    rows = {p: NONFINITE_KINDS[k % 4] for k, p in enumerate(NONFINITE_AT) if p < n}
    return build(n, pairs=ps, triples=ts, rotated=rotated, nonfinite=rows)


def nonfinite_keep(sc):
    """what the oracle does with the scene (tests/test_nms_scenes_cpu.py): the builder's list -- every non-finite row is a kept
    singleton -- but for the axis-aligned chain, where a row with a NaN x falls to the first box on its row of sites"""
    if sc.rotated:
        return sc.keep
    nan_x = [p for k, p in enumerate(NONFINITE_AT) if p < sc.n and NONFINITE_KINDS[k % 4] == "nan_centre"]
    return np.setdiff1d(sc.keep, nan_x)


# ------------------------------------------------------------------------------------------------------------- special geometry
def special_geometry():
    """-> [(name, box a, box b, closed-form IoU)].  Origin-centred shapes at indices 0, 4, 5, 6, 7: laid out cyclically
    (special_layout) rows and columns 0, 14, 15, 16, 31, 32 of the pairwise matrix hold non-zero values."""
    base = [0, 0, 0, 4, 2, 1.5, 0]
    far = [1504.0, -1496.0, 0, 4, 2, 1.5, 0]
    return [
        ("identical", base, base, 1.0),
        ("shared edge", base, [4, 0, 0, 4, 2, 1.5, 0], 0.0),
        ("corner touch", base, [4, 2, 0, 4, 2, 1.5, 0], 0.0),
        ("site around 1500", far, [far[0] + 1.5] + far[1:], 5.0 / 11.0),
        ("contained", base, [0, 0, 0, 2, 1, 1.5, 0], 0.25),
        ("cross", base, [0, 0, 0, 1, 4, 1.5, 0], 0.2),
        ("heading pi", base, [0, 0, 0, 4, 2, 1.5, np.pi], 1.0),
        ("heading pi/2, dimensions swapped", base, [0, 0, 0, 2, 4, 1.5, np.pi / 2], 1.0),
    ]


def special_layout(na, nb):
    sp = special_geometry()
    a = np.array([sp[i % len(sp)][1] for i in range(na)], np.float32).reshape(-1, 7)
    b = np.array([sp[j % len(sp)][2] for j in range(nb)], np.float32).reshape(-1, 7)
    return a, b


def tile_edges_nonzero(m, tile=16):
    """every tile of the (na, nb) matrix m has a non-zero value on its first and last row and its first and last column"""
    na, nb = m.shape
    for r0 in range(0, na, tile):
        for c0 in range(0, nb, tile):
            t = m[r0:r0 + tile, c0:c0 + tile]
            if not (np.any(t[0] != 0) and np.any(t[-1] != 0) and np.any(t[:, 0] != 0) and np.any(t[:, -1] != 0)):
                return False
    return True


def all_scenes(max_n=None):
    """[(name, thunk)] of every scene the tests use (the CPU test walks them all)"""
    out = []
    for rot in (True, False):
        r = "rot" if rot else "axis"
        for n in SMALL_N:
            out.append(("small-%d-%s" % (n, r), functools.partial(small, n, rot, True)))
        for n in (WORD_EDGE_N, CAP_N, 900):
            out.append(("word_edges-%d-%s" % (n, r), functools.partial(word_edges, rot, n)))
        out.append(("triples-%s" % r, functools.partial(triples, rot)))
        out.append(("piles-%s" % r, functools.partial(piles, rot)))
        out.append(("long-%s" % r, functools.partial(long_scene, rot)))
        for n in CHUNK_N:
            for v in (0, 1):
                out.append(("chunk-%d-v%d-%s" % (n, v, r), functools.partial(chunk_edges, n, v, rot)))
        for v in (0, 1, 2):
            out.append(("last_slot-v%d-%s" % (v, r), functools.partial(last_slot, v, rot)))
        for M in CAPS:
            for kind in cap_kinds(M):
                out.append(("cap-%d-%s-%s" % (M, kind, r), functools.partial(cap, M, kind, rot)))
        for v in (0, 1):
            out.append(("fill4096-v%d-%s" % (v, r), functools.partial(fill4096, v, rot)))
        for w in (0, 1, 2):
            out.append(("three-%d-%s" % (w, r), functools.partial(three, w, rot)))
        for m in FUSED_M:
            out.append(("fused-%d-%s" % (m, r), functools.partial(fused, m, rot)))
    return out
