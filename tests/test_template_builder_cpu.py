"""btcdet_amd/template_builder.py without a GPU: the numpy restatement of include/btcdet_hip_templates.h (template_ref.restate_*) against
the vectors the reference's own multifindbestfit.py functions produced (tests/golden/templates.npz) and against a float64 brute force,
the host stages and host pieces of TemplateBuilder, and the C ABI's table and argument checks."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

import template_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "templates.npz")
CLASSES = ("Car", "Cyclist", "Pedestrian")


@pytest.fixture(scope="module")
def golds():
    return {name: tr.load_golden(GOLD, name) for name in CLASSES}


@pytest.fixture(scope="module")
def sets(golds):
    return {name: tr.golden_sets(golds[name], name) for name in CLASSES}


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("top_k", [3, 5])
@pytest.mark.parametrize("name", CLASSES)
def test_restatement_reproduces_the_reference(golds, sets, name, top_k):
    """selection, order and counts exactly; coordinates within 1 float32 ulp (the reference rotates with a BLAS matmul in double, whose
    summation order is not defined, and rounds when it pickles)"""
    gold, run = golds[name], golds[name]["runs"][top_k]
    assert [s.shape[0] for s in sets[name]] == run["set_counts"].tolist()
    res = tr.restate_class(sets[name], gold["boxes"], tr.CLASS_PARAMS[name], top_k)
    assert res["cand"].tolist() == run["cand"].tolist()
    assert np.abs(res["iou"] - run["iou"]).max() == 0
    assert res["chosen"].tolist() == run["chosen"].tolist()
    assert [t.shape[0] for t in res["templates"]] == [t.shape[0] for t in run["templates"]]
    for j, (mine, want) in enumerate(zip(res["templates"], run["templates"])):
        assert want.dtype == np.float32 and tr.ulp_apart(mine, want) <= 1, (name, top_k, j)
        at, src = int(run["set_counts"][j]), res["src"][j]
        assert (src[:at, 0] == j).all() and src[:at, 1].tolist() == list(range(at))          # the object's own set comes first
        for c, n in zip(run["chosen"][j], run["added"][j]):                                   # then what every round appended, in order
            assert (n > 4) == (c >= 0)
            if c >= 0:
                assert (src[at:at + n, 0] == c).all() and (np.diff(src[at:at + n, 1]) > 0).all()
                at += int(n)
        assert at == want.shape[0]
    assert (run["chosen"] >= 0).any() and (name != "Car" or (run["chosen"] < 0).any()), "rounds that appended rows, and for Car rounds that did not"


@pytest.mark.parametrize("name", CLASSES)
def test_restatement_equals_the_float64_brute_force_on_decisions(golds, sets, name):
    gold = golds[name]
    iou = tr.box_iou_origin(gold["boxes"][:, 3:6])
    for top_k in (1, 3, 5, 800):
        res = tr.restate_class(sets[name], gold["boxes"], tr.CLASS_PARAMS[name], top_k, iou)
        chosen, segs = tr.brute_class(sets[name], gold["boxes"], tr.CLASS_PARAMS[name], top_k, iou)
        assert res["chosen"].tolist() == chosen.tolist()
        for j, s in enumerate(segs):
            want = np.concatenate([np.stack([np.full(len(r), c), r], axis=1) for c, r in s]).astype(np.int32)
            assert np.array_equal(res["src"][j], want), (name, top_k, j)


def test_nearest_sq_is_the_square_root_decision():
    from btcdet_amd.template_builder import nearest_sq
    for nd in (0.05, 0.10, 0.16, 1.0):
        t = nearest_sq(nd)
        assert t == tr.nearest_sq(nd) and t.dtype == np.float32
        assert np.sqrt(t) <= np.float32(nd) < np.sqrt(np.nextafter(t, np.float32(np.inf)))


def test_cells_on_the_last_edge_and_faces(sets):
    from btcdet_amd.template_builder import grid_of
    for name in CLASSES:                                         # the builder's grid is the restatement's
        cat = np.concatenate(sets[name])
        mine, want = grid_of(cat[:, :2].min(axis=0), cat[:, :2].max(axis=0), 0.16), tr.make_grid(sets[name])
        assert mine == want and all(type(mine[k]) is type(want[k]) for k in want)
    assert grid_of(None, None, 0.16) == tr.make_grid([np.zeros((0, 3), np.float32)])
    assert grid_of(np.float32([0, 0]), np.float32([0.32, 0]), 0.16)["nx"] == int(np.ceil(float(np.float32(0.32)) / 0.16)) and grid_of([0, 0], [0, 0], 0.16)["ny"] == 1
    grid = dict(x0=np.float32(0), y0=np.float32(0), cell=np.float32(0.5), nx=2, ny=3)
    pts = np.array([[0, 0, 0], [0.5, 1.0, 0], [1.0, 0.2, 0], [0.2, 1.5, 0], [0.99, 1.49, 5]], np.float32)   # rows 2 and 3 sit on index nx / ny
    assert tr.occ_words(pts, grid).tolist() == [(1 << 0) | (1 << 5)]
    md, so = tr.restate_match([pts[:2], pts], [np.array([0.5, 1.0, 0.0], np.float32)] * 2, np.array([0]), np.array([[1]]), grid)
    assert so[0, 0].tolist() == [(1 << 0) | (1 << 5)] and md[0, 0] == 0      # faces inclusive: (0.5, 1.0, 0) is inside


# ------------------------------------------------------------------------------------------------------------ host pieces of the builder
def test_normalise_on_the_host_route_and_in_torch(golds):
    """step 1 as TemplateBuilder does it (torch double on the bank's device, here the CPU) equals the restatement bit for bit; a float32
    box takes normalize_host, the reference's expressions under numpy's promotion: float32 throughout"""
    from btcdet_amd.template_builder import TemplateBuilder, normalize_host
    gold = golds["Car"]
    tb = TemplateBuilder(tr.golden_databases({"Car": gold}), device="cpu")
    objs = tb.class_objects("Car")
    assert [int(o[1]["image_idx"]) for o in objs] == gold["image_idx"].tolist()
    kept, oid, counts = tb.normalized_sets(objs)
    want = [tr.restate_normalize(r, b) for r, b in zip(gold["rows"], gold["boxes"])]
    assert counts.tolist() == [w.shape[0] for w in want] and kept.numpy().tobytes() == np.concatenate(want).tobytes()
    assert oid.tolist() == np.repeat(np.arange(len(want)), counts).tolist()
    tb32 = TemplateBuilder(tr.golden_databases({"Car": gold}, box_dtype=np.float32), device="cpu")
    kept32, _, counts32 = tb32.normalized_sets(tb32.class_objects("Car"))
    host = [normalize_host(r, b.astype(np.float32), 0.15) for r, b in zip(gold["rows"], gold["boxes"])]
    want32 = [tr.restate_normalize(r, b.astype(np.float32)) for r, b in zip(gold["rows"], gold["boxes"])]
    assert counts32.tolist() == [h.shape[0] for h in host] and kept32.numpy().tobytes() == np.concatenate(host).tobytes() == np.concatenate(want32).tobytes()
    # against the reference's form of the same sums, a float32 matmul whose order and contraction BLAS does not define: each
    # coordinate is a difference or sum of two products, so the two can differ by the rounding of one product and of the sum --
    # 2 float32 steps of the larger product
    j = int(np.argmax(counts))
    b32 = gold["boxes"][j].astype(np.float32)
    c, s = np.cos(-b32[6]), np.sin(-b32[6])
    assert c.dtype == np.float32
    p = gold["rows"][j][:, :3]
    p = p[p[:, 2] > (-b32[5] / 2 + 0.15)]
    blas = np.matmul(p, np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]], np.float32))
    bound = 2 * np.spacing(np.abs(p[:, :2]).max(axis=1) * max(abs(c), abs(s)))
    assert blas.dtype == np.float32 and (np.abs(host[j][:, :2] - blas[:, :2]) <= bound[:, None]).all() and np.array_equal(host[j][:, 2], p[:, 2])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["device_route", "host_route"])
def test_the_bottom_cut_at_equality(dtype):
    """rows exactly on z = -dz/2 + bottom are cut, one float32 step above stays, one below goes -- here with torch on the CPU"""
    from btcdet_amd.template_builder import TemplateBuilder
    db, rows, boxes, keep = tr.bottom_database(dtype)
    tb = TemplateBuilder([db], device="cpu")
    kept, oid, counts = tb.normalized_sets(tb.class_objects("Car"))
    want = [tr.restate_normalize(r, b) for r, b in zip(rows, boxes)]
    assert counts.tolist() == [int(keep.sum()), want[1].shape[0]] and kept.numpy().tobytes() == np.concatenate(want).tobytes()
    thr = -boxes[0][5] / 2 + 0.15
    assert (kept.numpy()[:counts[0], 2] > thr).all() and (rows[0][:, 2] == thr).sum() == 3


def test_batching_by_budget_and_names():
    from btcdet_amd.template_builder import CLASS_PARAMS, TemplateBuilder, batch_objects, directory_name, file_name
    per = 800 * 23 * 4 + 800 * 12 + 14000 * 16
    assert batch_objects(10 * per, 800, 23, 14000, 28000) == 10 and batch_objects(10 * per - 1, 800, 23, 14000, 28000) == 9
    more = per + 2 * 3000 + 3 * 3000 * 12                         # the select workspace's flag bytes and the template rows at their bound
    assert batch_objects(10 * more, 800, 23, 14000, 28000, 2, 3000) == 10 and batch_objects(10 * more - 1, 800, 23, 14000, 28000, 2, 3000) == 9
    assert batch_objects(1, 800, 23, 14000, 28000) == 1 and batch_objects(1 << 40, 800, 23, 14000, 50) == 50
    assert CLASS_PARAMS == tr.CLASS_PARAMS
    assert [directory_name(n, CLASS_PARAMS[n]) for n in CLASSES] == ["bm_50maxdist_2num_Car", "bm_5maxdist_1num_Cyclist", "bm_5maxdist_1num_Pedestrian"]
    assert file_name({"image_idx": "000123", "gt_idx": 4}) == "123_4.pkl"
    tb = TemplateBuilder([], class_params={"Cyclist": {"max_num_bm": 2}, "Van": dict(mirror=True, pnt_thresh=9, ex_coords_ratio=7, max_num_bm=3, nearest_dist=0.1)})
    assert directory_name("Cyclist", tb.class_params["Cyclist"]) == "bm_5maxdist_2num_Cyclist" and tb.class_params["Cyclist"]["pnt_thresh"] == 5
    assert directory_name("Van", tb.class_params["Van"]) == "bm_7maxdist_3num_Van" and tb.top_k == 800
    with pytest.raises(ValueError):
        TemplateBuilder([], class_params={"Car": {"max_num_bm": 9}})
    with pytest.raises(KeyError):
        tb.build_class("Truck")
    with pytest.raises(ValueError):
        tb.save("/nonexistent")


def test_save_and_read_back(tmp_path, golds):
    """save() writes what TemplateBank(template_root) and the reference's querier read: a pickled float32 (n, 3) array per object"""
    from btcdet_amd.device_augmentor import TemplateBank
    from btcdet_amd.template_builder import TemplateBuilder, directory_name
    tb = TemplateBuilder(tr.golden_databases(golds), device="cpu")
    table, parts, first = {}, [], 0
    for name in CLASSES:
        tb.infos[name] = [o[1] for o in tb.class_objects(name)]
        for info, t in zip(tb.infos[name], golds[name]["runs"][3]["templates"]):
            table[(name, int(info["image_idx"]), int(info["gt_idx"]))] = (first, t.shape[0])
            parts.append(t)
            first += t.shape[0]
    tb.bank, tb.built = TemplateBank.from_rows(np.concatenate(parts), table), list(CLASSES)
    dirs = tb.save(tmp_path)
    assert sorted(os.listdir(tmp_path)) == sorted(directory_name(n, tb.class_params[n]) for n in CLASSES)
    back = TemplateBank({n: str(d) for n, d in dirs.items()})
    assert sorted(back.table) == sorted(table) and back.nbytes == tb.bank.nbytes == first * 12
    for k, (f, n) in table.items():
        bf, bn = back.table[k]
        assert bn == n and back.rows[bf:bf + bn].tobytes() == tb.bank.rows[f:f + n].tobytes()
    info = tb.infos["Car"][0]
    with open(dirs["Car"] / ("%d_%d.pkl" % (int(info["image_idx"]), int(info["gt_idx"]))), "rb") as f:
        a = pickle.load(f)
    assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 3
    res = TemplateBank.from_rows(None, table, device_rows=torch.from_numpy(np.concatenate(parts)))       # a resident bank: tensor() is the rows
    assert res.tensor("cpu") is res._resident and res.rows.tobytes() == tb.bank.rows.tobytes() and res.load_point_features == 3
    with pytest.raises(ValueError):
        TemplateBank.from_rows(None, table)


# ------------------------------------------------------------------------------------------------------------------------- C ABI
SYMBOLS = ["btc_match_candidates", "btc_nn_sqdist", "btc_select_templates", "btc_select_templates_ws_bytes"]


def test_ctypes_table_matches_the_header():
    from btcdet_amd import _lib
    src = open(os.path.join(ROOT, "include", "btcdet_hip_templates.h")).read()
    for line in ("d2 = ((dx*dx) + (dy*dy)) + (dz*dz)", "ix = floor((x - x0) / cell), iy = floor((y - y0) / cell)",
                 "h[k]     = ((max_dist[g][k] + ratio / extra[k]) + (iou[g][k] < iou_thresh ? 2 : 0)) + (extra[k] < 30 ? 1 : 0)"):
        assert line in src, "the header states its formulas: " + line
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(btc_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib.TEMPLATES_EXPORTED_SYMBOLS) == SYMBOLS
    L = _lib.lib()
    kinds = {"int": _lib.ci, "size_t": _lib.sz, "float": _lib.cf}
    for n, count in (("btc_nn_sqdist", 10), ("btc_match_candidates", 17), ("btc_select_templates_ws_bytes", 3), ("btc_select_templates", 27)):
        assert hasattr(L, n)
        res, args = _lib._TEMPLATES_SIGS[n]
        m = re.search(r"(size_t|int)\s+%s\s*\(([^)]*)\)" % n, src)
        assert kinds[m.group(1)] is res, n
        params = [p.strip() for p in m.group(2).split(",")]
        assert len(params) == len(args) == count, n
        for p, a in zip(params, args):
            want = _lib.vp if "*" in p else kinds[re.sub(r"\s+\w+$", "", p).replace("const ", "").strip()]
            assert a is want, (n, p)
    for other in ("btcdet_hip.h", "btcdet_hip_infer.h", "btcdet_hip_augment.h", "btcdet_hip_bestmatch.h", "btcdet_hip_frames.h", "btcdet_hip_gtdb.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(s + "(" in text for s in SYMBOLS)
    assert "btcdet_hip_templates.h" in open(os.path.join(ROOT, "btcdet_amd", "csrc", "Makefile")).read()


P = 0x1000      # a non-null address nobody reads: every call below returns from its argument checks


def test_argument_checks_return_before_any_launch():
    from btcdet_amd import _lib
    L = _lib.lib()
    nn = dict(q=P, nq=8, t=P, nt=8, pairs=P, offs=P, P=2, out_rows=8, out=P)
    for kw in (dict(P=-1), dict(nq=-1), dict(nt=-1), dict(out_rows=-1), dict(pairs=None), dict(offs=None), dict(q=None), dict(t=None), dict(out=None)):
        assert L.btc_nn_sqdist(*dict(nn, **kw).values(), None) == -1, kw
    assert b"btc_nn_sqdist" in L.btc_last_error()
    mc = dict(points=P, n=8, seg=P, half=P, M=2, obj=P, cand=P, G=2, K=3, x0=0.0, y0=0.0, cell=0.16, nx=4, ny=8, md=P, so=P)
    for kw in (dict(n=-1), dict(M=-1), dict(G=-1), dict(K=0), dict(nx=0), dict(ny=0), dict(cell=0.0), dict(cell=-1.0), dict(nx=2048, ny=33),
               dict(points=None), dict(seg=None), dict(half=None), dict(obj=None), dict(cand=None), dict(md=None), dict(so=None),
               dict(G=1 << 20, K=1 << 12)):
        assert L.btc_match_candidates(*dict(mc, **kw).values(), None) == -1, kw
    assert L.btc_select_templates_ws_bytes(4, 2, 300) >= 4 * 2 * 300 + 4 * 4
    for bad in ((-1, 2, 300), (4, 0, 300), (4, 9, 300), (4, 2, -1), (1 << 20, 8, 1 << 10)):
        assert L.btc_select_templates_ws_bytes(*bad) == 0, bad
    ws = L.btc_select_templates_ws_bytes(2, 2, 16)
    st = dict(points=P, n=8, seg=P, M=2, obj=P, cand=P, iou=P, md=P, so=P, own=P, G=2, K=3, W=1, nbm=2, extra=2000, thr=0.9, ratio=50.0, nsq=0.01,
              max_rows=16, cap=8, out=P, src=P, offs=P, chosen=P, ws=P, ws_bytes=ws)
    for kw in (dict(G=-1), dict(M=-1), dict(n=-1), dict(cap=-1), dict(max_rows=-1), dict(extra=-1), dict(K=0), dict(K=8193), dict(W=0), dict(W=2049),
               dict(nbm=0), dict(nbm=9), dict(offs=None), dict(chosen=None), dict(ws=None), dict(obj=None), dict(cand=None), dict(iou=None), dict(md=None),
               dict(so=None), dict(seg=None), dict(own=None), dict(points=None), dict(out=None), dict(ws_bytes=ws - 1), dict(ws_bytes=0),
               dict(max_rows=4096)):
        assert L.btc_select_templates(*dict(st, **kw).values(), None) == -1, kw
    assert b"btc_select_templates" in L.btc_last_error()
