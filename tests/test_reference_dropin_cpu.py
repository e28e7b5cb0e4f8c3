"""Drop-in check against the reference's OWN backbone file: the reference tree's btcdet/models/backbones_3d/spconv_backbone.py imports
`spconv`; with btcdet_amd.install_as_spconv() it imports THIS implementation, its classes construct on top of it, and their
state_dict (keys, shapes) is identical to the one of this repository's backbones, so reference checkpoints load key-for-key.
Where the reference tree is not there, every test checks this repository against what the reference's modules recorded
(tests/golden/ref_dropin.json, tests/golden/ref_state_keys.json); where it is, against the live modules, and the recordings
must still be current (tests/golden/gen_dropin_golden.py regenerates ref_dropin.json)."""
import importlib
import importlib.util
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

REF = "/root/reference/btcdet/models/backbones_3d/spconv_backbone.py"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorded():
    with open(os.path.join(GOLDEN, "ref_dropin.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ref_mod():
    """the reference's spconv_backbone module built on this spconv, or None where the reference tree is not there"""
    import btcdet_amd
    if not os.path.exists(REF):
        yield None
        return
    saved = {k: sys.modules.get(k) for k in ("spconv", "spconv.utils", "spconv.ops")}
    btcdet_amd.install_as_spconv()
    spec = importlib.util.spec_from_file_location("_ref_spconv_backbone", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    yield mod
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def _cfgs():
    from btcdet_amd.config import load_cfg
    cfg = load_cfg()
    return cfg, cfg.MODEL.OCC.BACKBONE_3D, cfg.MODEL.BACKBONE_3D


def _occ_kw():
    cfg, occ_cfg, _ = _cfgs()
    return dict(model_cfg=occ_cfg, input_channels=4, grid_size=np.array([209, 157, 9]), voxel_size=[0.32, 0.5184, 0.36],
                point_cloud_range=cfg.DATA_CONFIG.POINT_CLOUD_RANGE, original_num_rawpoint_features=4)


def _det_kw():
    cfg, _, det_cfg = _cfgs()
    return dict(model_cfg=det_cfg, input_channels=6, grid_size=np.array([1408, 1600, 40]), voxel_size=[0.05, 0.05, 0.1],
                point_cloud_range=cfg.DATA_CONFIG.POINT_CLOUD_RANGE, original_num_rawpoint_features=4)


def _variant_kw(cin, grid):
    _, occ_cfg, _ = _cfgs()
    return dict(model_cfg=occ_cfg, input_channels=cin, grid_size=np.array(grid))


VARIANTS = [("VoxelBackBoneDeconvRes", 4, [209, 157, 9]), ("VoxelBackBoneInverseRes", 4, [209, 157, 9]), ("VoxelResBackBone8x", 4, [1408, 1600, 40])]


def _norm_fn():
    from functools import partial
    return partial(torch.nn.BatchNorm1d, eps=1e-3, momentum=0.01)


def _block_args():
    return (16, 32, 3), dict(indice_key="k", stride=2, padding=1, conv_type="spconv", norm_fn=lambda c: torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01))


def record(m):
    """what a test compares of a module: state_dict keys, shapes and dtypes in order (+ the backbones' output description)"""
    out = {"state": [[k, list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()]}
    if hasattr(m, "num_point_features"):
        out["num_point_features"] = m.num_point_features
    if hasattr(m, "sparse_shape"):
        out["sparse_shape"] = [int(s) for s in m.sparse_shape]
    return out


def record_block(blk):
    return {"types": [type(blk).__name__] + [type(c).__name__ for c in blk], "weight_shape": list(blk[0].weight.shape), **record(blk)}


def reference_modules(ref_mod, p2_mods):
    """name -> the reference's module of each comparison (tests/golden/gen_dropin_golden.py records them)"""
    out = {"post_act_block": ref_mod.post_act_block(*_block_args()[0], **_block_args()[1]),
           "VoxelBackBoneDeconv": ref_mod.VoxelBackBoneDeconv(**_occ_kw()),
           "VoxelBackBone8xOcc": ref_mod.VoxelBackBone8xOcc(**_det_kw()),
           "SparseBasicBlock": ref_mod.SparseBasicBlock(32, 32, norm_fn=_norm_fn(), indice_key="res2")}
    for name, cin, grid in VARIANTS:
        out[name] = getattr(ref_mod, name)(**_variant_kw(cin, grid))
    out.update(_pointnet2_ref_modules(p2_mods))
    return out


def _pointnet2_ref_modules(mods):
    kw = dict(radii=[0.8, 1.6], nsamples=[16, 16], use_xyz=True, pool_method="max_pool")
    return {"StackSAModuleMSG": mods["pointnet2_modules"].StackSAModuleMSG(mlps=[[1, 16, 16], [1, 16, 16]], **kw),
            "StackPointnetFPModule": mods["pointnet2_modules"].StackPointnetFPModule(mlp=[32, 16])}


def _reference(ref_mod, name, build):
    """the reference's record of one comparison: from the live module where the reference is there (the recording must be current),
    else the recording"""
    rec = _recorded()[name]
    if ref_mod is None:
        return rec, None
    live = build(ref_mod)
    assert json.loads(json.dumps(record_block(live) if name == "post_act_block" else record(live))) == rec, \
        "tests/golden/ref_dropin.json is stale: python tests/golden/gen_dropin_golden.py"
    return rec, live


def _same_state(mine, rec, live=None):
    a = mine.state_dict()
    assert list(a.keys()) == [k for k, _, _ in rec["state"]]
    for k, shape, _ in rec["state"]:
        assert list(a[k].shape) == shape, k
    if live is not None:
        mine.load_state_dict(live.state_dict(), strict=True)
    else:
        mine.load_state_dict({k: torch.zeros(shape, dtype=getattr(torch, dt.split(".")[-1])) for k, shape, dt in rec["state"]}, strict=True)


def test_reference_module_uses_this_spconv(ref_mod):
    import btcdet_amd
    import btcdet_amd.spconv as sp
    from btcdet_amd import backbones_3d
    rec, live = _reference(ref_mod, "post_act_block", lambda r: r.post_act_block(*_block_args()[0], **_block_args()[1]))
    if ref_mod is not None:
        assert ref_mod.spconv is sp
        blk = live
    else:   # the module the reference's `import spconv` gets, and this repository's block built as the reference built its own
        saved = {k: sys.modules.get(k) for k in ("spconv", "spconv.utils", "spconv.ops")}
        try:
            btcdet_amd.install_as_spconv()
            assert importlib.import_module("spconv") is sp and importlib.import_module("spconv.utils") is sp.utils
        finally:
            for k, v in saved.items():
                if v is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = v
        blk = backbones_3d.post_act_block(*_block_args()[0], **_block_args()[1])
        assert record_block(blk)["types"] == rec["types"]
        _same_state(blk, rec)
    assert isinstance(blk, sp.SparseSequential) and isinstance(blk[0], sp.SparseConv3d)
    assert tuple(blk[0].weight.shape) == (3, 3, 3, 16, 32) and list(blk[0].weight.shape) == rec["weight_shape"]


def _backbone_matches(ref_mod, name, build_ref, mine):
    rec, live = _reference(ref_mod, name, build_ref)
    _same_state(mine, rec, live)
    assert mine.num_point_features == rec["num_point_features"]
    assert [int(s) for s in mine.sparse_shape] == rec["sparse_shape"]


def test_occupancy_backbone_state_dict_matches_reference(ref_mod):
    from btcdet_amd import backbones_3d
    _backbone_matches(ref_mod, "VoxelBackBoneDeconv", lambda r: r.VoxelBackBoneDeconv(**_occ_kw()), backbones_3d.VoxelBackBoneDeconv(**_occ_kw()))


def test_detection_backbone_state_dict_matches_reference(ref_mod):
    from btcdet_amd import backbones_3d
    _backbone_matches(ref_mod, "VoxelBackBone8xOcc", lambda r: r.VoxelBackBone8xOcc(**_det_kw()), backbones_3d.VoxelBackBone8xOcc(**_det_kw()))


@pytest.mark.parametrize("name,cin,grid", VARIANTS)
def test_unconfigured_backbone_variants_match_reference(ref_mod, name, cin, grid, capsys):
    """the variants reachable through BACKBONE_3D.NAME"""
    from btcdet_amd import backbones_3d
    _backbone_matches(ref_mod, name, lambda r: getattr(r, name)(**_variant_kw(cin, grid)), backbones_3d.__all__[name](**_variant_kw(cin, grid)))


def test_sparse_basic_block_matches_reference(ref_mod):
    from btcdet_amd import backbones_3d
    rec, live = _reference(ref_mod, "SparseBasicBlock", lambda r: r.SparseBasicBlock(32, 32, norm_fn=_norm_fn(), indice_key="res2"))
    _same_state(backbones_3d.SparseBasicBlock(32, 32, norm_fn=_norm_fn(), indice_key="res2"), rec, live)


HOT = ("occ_modules.", "det_modules.vfe", "det_modules.backbone_3d", "det_modules.map_to_bev_module", "global_step")


def _hot_path_state():
    from btcdet_amd.btc_path import BtcHotPath
    from btcdet_amd.config import load_cfg
    return {k: list(v.shape) for k, v in BtcHotPath(load_cfg(), device="cpu").state_dict().items()}


def test_reference_btcnet_builds_on_this_spconv_and_hot_path_state_dict_matches():
    """the reference's OWN BtcNet (detector template, registries, yaml) constructs with `spconv` = btcdet_amd.spconv; the
    hot-path part of its state_dict (occ_modules.*, det_modules.{vfe, backbone_3d, map_to_bev_module}) equals BtcHotPath's
    key for key, shape for shape, in order -- so a reference checkpoint loads into the hot path and vice versa"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    committed = json.load(open(os.path.join(root, "tests", "golden", "ref_state_keys.json")))
    if os.path.exists(REF):
        out = subprocess.run([sys.executable, os.path.join(root, "tests", "golden", "ref_build_state.py")], capture_output=True, timeout=600)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        res = json.loads(out.stdout.decode().strip().splitlines()[-1])
        assert committed["keys"] == res["keys"]  # the fixture used where the reference is not there is current
    else:
        res = committed
    # the reference's iou3d_nms_utils.py imported with its compiled module resolved to btcdet_amd.iou3d_nms.iou3d_nms_cuda
    assert res["iou3d_nms_utils_bound_to_btcdet_amd"] is True
    ref = res["keys"]
    assert len(ref) > 300  # the whole detector built, incl. the out-of-scope 2-D backbone and heads
    hot = {k: v for k, v in ref.items() if k.startswith(HOT)}
    mine = _hot_path_state()
    assert list(hot.keys()) == list(mine.keys())
    assert hot == mine


PN2_PKG = "btcdet.ops.pointnet2.pointnet2_stack"
PN2_ROOT = os.path.join(REF[:REF.index("/btcdet/models/")], "btcdet", "ops", "pointnet2", "pointnet2_stack")   # (same reference tree)


def load_reference_pointnet2(p2):
    """the reference's pointnet2_utils.py / pointnet2_modules.py loaded with `pointnet2_stack_cuda` = this implementation's stand-in
    -> (stand-in, {file name: module}); the caller restores sys.modules"""
    parts = PN2_PKG.split(".")
    for i in range(1, len(parts) + 1):
        name = ".".join(parts[:i])
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    stand_in = p2.install_as_pointnet2_stack_cuda(PN2_PKG)
    mods = {}
    if os.path.exists(PN2_ROOT):
        for fname in ("pointnet2_utils", "pointnet2_modules"):
            spec = importlib.util.spec_from_file_location(PN2_PKG + "." + fname, os.path.join(PN2_ROOT, fname + ".py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[PN2_PKG + "." + fname] = mod
            setattr(sys.modules[PN2_PKG], fname, mod)
            spec.loader.exec_module(mod)
            mods[fname] = mod
    return stand_in, mods


def test_reference_pointnet2_stack_binds_the_stand_in():
    """the reference's pointnet2_utils.py / pointnet2_modules.py import `pointnet2_stack_cuda`; with
    btcdet_amd.pointnet2_stack.install_as_pointnet2_stack_cuda() they import this implementation's entry points, and the
    reference's StackSAModuleMSG has the same parameters as this repository's"""
    from btcdet_amd import pointnet2_stack as p2
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k == "btcdet" or k.startswith("btcdet.")}
    try:
        stand_in, mods = load_reference_pointnet2(p2)
        # what the reference's `from . import pointnet2_stack_cuda as pointnet2` gets
        assert importlib.import_module(PN2_PKG + ".pointnet2_stack_cuda") is stand_in
        if mods:
            assert mods["pointnet2_utils"].pointnet2 is stand_in
        for name in ("ball_query_wrapper", "shell_query_wrapper", "group_points_wrapper", "group_points_grad_wrapper",
                     "furthest_point_sampling_wrapper", "three_nn_wrapper", "three_interpolate_wrapper", "three_interpolate_grad_wrapper"):
            assert callable(getattr(stand_in, name))
        live = _pointnet2_ref_modules(mods) if mods else {}
        kw = dict(radii=[0.8, 1.6], nsamples=[16, 16], use_xyz=True, pool_method="max_pool")
        for name, mine in (("StackSAModuleMSG", p2.StackSAModuleMSG(mlps=[[1, 16, 16], [1, 16, 16]], **kw)),
                           ("StackPointnetFPModule", p2.StackPointnetFPModule(mlp=[32, 16]))):
            rec, lv = _reference(live or None, name, lambda r: r[name])
            _same_state(mine, rec, lv)
    finally:
        for k in [k for k in sys.modules if k == "btcdet" or k.startswith("btcdet.")]:
            sys.modules.pop(k, None)
        for k, v in saved.items():
            if v is not None:
                sys.modules[k] = v
