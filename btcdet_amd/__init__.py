"""btcdet_amd -- MI355X (gfx950) implementation of BtcDet's data-parallel hot path.

Voxelizer, occupancy/occlusion target generator, sparse-3D-conv rulebook + fused gather-GEMM-scatter
(forward and backward), exposed through the reference's own operator / module API:

* ``btcdet_amd.spconv``         -- drop-in for the ``spconv`` v1.2.1 surface BtcDet uses
* ``btcdet_amd.processor``      -- ``DataProcessor`` voxelization steps on the GPU
* ``btcdet_amd.device_augmentor`` -- ``DataAugmentor`` (host protocol) and ``DeviceAugmentor``: paste, flip, scale, rotate on a resident batch;
  ``TemplateBank``: best-match templates resident, ``bm_points`` placed in one launch
* ``btcdet_amd.kitti_frames``   -- ``KittiFrames`` / ``Calibration``: a KITTI directory into a resident batch, the FOV crop on the GPU
* ``btcdet_amd.gt_database``    -- ``GtDatabase``: the ground-truth database of ``gt_sampling`` cut from resident scans, its bank resident
* ``btcdet_amd.template_builder`` -- ``TemplateBuilder``: the best-match templates made from resident databases, their bank resident
* ``btcdet_amd.kitti_infos``    -- ``KittiInfoBuilder`` / ``add_coverage``: the info pickles from a raw KITTI directory, points per box and
  coverage cells counted on the GPU
* ``btcdet_amd.anchor_targets`` -- ``DeviceTargetAssigner`` / ``decode_boxes``: the anchor head's targets and boxes in four launches (opt-in)
* ``btcdet_amd.anchor_loss``    -- ``anchor_loss``: the anchor head's loss, one launch forward and one backward (opt-in)
* ``btcdet_amd.roi_targets_device`` -- ``DeviceProposalTargets``: the ROI head's targets (matching, sampling, canonical transform) in one launch (opt-in)
* ``btcdet_amd.roi_loss``       -- ``roi_loss``: the ROI head's loss, one launch forward and one backward (opt-in)
* ``btcdet_amd.occ_targets``    -- ``OccTargets3D`` (occupancy / occlusion grid generator)
* ``btcdet_amd.vfe`` / ``backbones_3d`` / ``occ_head`` / ``pass_occ_vox`` / ``height_compression``

All compute goes through ``libbtcdet_hip.so`` (hand-written HIP, C ABI in ``include/btcdet_hip.h``, ``btcdet_hip_infer.h``,
``btcdet_hip_augment.h``, ``btcdet_hip_bestmatch.h``, ``btcdet_hip_frames.h``, ``btcdet_hip_gtdb.h``, ``btcdet_hip_templates.h``,
``btcdet_hip_infos.h``, ``btcdet_hip_heads.h``, ``btcdet_hip_anchor_loss.h``, ``btcdet_hip_roi_targets.h``, ``btcdet_hip_roi_loss.h``).
"""
__version__ = "0.1.0"


def install_as_spconv():
    """Register ``btcdet_amd.spconv`` under the module name ``spconv`` so that the reference's
    ``import spconv`` / ``from spconv.utils import VoxelGeneratorV2`` resolve to this implementation
    (/root/reference/btcdet/models/backbones_3d/spconv_backbone.py:3, data_processor.py:64)."""
    import sys
    from . import spconv as _sp
    sys.modules["spconv"] = _sp
    sys.modules["spconv.utils"] = _sp.utils
    sys.modules["spconv.ops"] = _sp.ops
    return _sp
