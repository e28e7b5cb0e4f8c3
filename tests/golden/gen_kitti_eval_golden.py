"""Golden vectors of the KITTI evaluation: the reference's OWN kitti_object_eval_python/eval.py (get_official_eval_result, eval_class
with clean_data, compute_statistics_jit, fused_compute_statistics, get_thresholds) executed here on CPU.

    python tests/golden/gen_kitti_eval_golden.py   ->  tests/golden/kitti_eval.npz

Two substitutions make it run: `numba.jit` is an identity decorator, and the module `rotate_iou` is replaced.  The reference's
rotate_iou.py is numba.cuda and executes on no machine this project has, so `rotate_iou_gpu_eval` is SERVED by the float64 convex
clipping of tests/kitti_eval_ref.py: the reference's matching, threshold and AP logic is executed as it is, on overlap values that are
exact geometry.  The overlap VALUES are therefore pinned to geometry, not to a run of the reference's CUDA kernel (which rounds its
boxes to float32 first).  eval.py is loaded by file path under a synthetic package, so btcdet.datasets' heavy imports are not needed.

Only expected outputs are stored (per case and metric the four [class, difficulty, level, 41] arrays, ret_dict, the result string);
the inputs are regenerated from seeds by kitti_eval_ref.make_case.  The annotation builder is pinned too: the reference's
box_utils.boxes3d_lidar_to_kitti_camera / boxes3d_kitti_camera_to_imageboxes with calibration_kitti.Calibration on seeded boxes.

The generator ASSERTS the margins that make exact decisions a fair demand (make_case redraws a frame that violates them):
  * no overlap within 1e-4 of an overlap level in use (0.7 / 0.5 / 0.25);
  * for any ground truth, no two candidate detections above the lowest level with overlaps closer than 2e-4;
  * no image-box height, truncation or coverage_rates value equal to a limit.
(The first two are at least twice the IoU tolerance the project uses, rtol 1e-4 / atol 2e-5.)"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_env  # noqa: E402
import oracle_spconv  # noqa: E402
import kitti_eval_ref as ref  # noqa: E402

EVAL_DIR = os.path.join(ref_env.REF, "btcdet", "datasets", "kitti", "kitti_object_eval_python")


def load_reference_eval():
    def jit(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda fn: fn

    sys.modules["numba"] = types.SimpleNamespace(jit=jit)
    pkg = types.ModuleType("koep")
    pkg.__path__ = [EVAL_DIR]
    sys.modules["koep"] = pkg
    rot = types.ModuleType("koep.rotate_iou")
    rot.rotate_iou_gpu_eval = lambda boxes, qboxes, criterion=-1, device_id=0: ref.rotate_iou_eval(boxes, qboxes, criterion)
    sys.modules["koep.rotate_iou"] = rot
    spec = importlib.util.spec_from_file_location("koep.eval", os.path.join(EVAL_DIR, "eval.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["koep.eval"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ev = load_reference_eval()
    out = {}
    meta = {}
    for name, (kw, classes, cov) in ref.GOLDEN_CASES.items():
        gt, dt = ref.make_case(**kw)
        w = ref.margins(gt, dt)
        print(name, "margins", {k: "%.3g" % v for k, v in w.items()})
        assert w["level"] >= ref.MARGIN["level"], (name, "an overlap within 1e-4 of a level", w)
        assert w["gap"] >= ref.MARGIN["gap"], (name, "two candidates of one ground truth closer than 2e-4", w)
        assert w["limit"] >= ref.MARGIN["limit"], (name, "a height / truncation / coverage value on a limit", w)
        classes_int = ref.classes_to_int(classes)
        mo = ref.official_min_overlaps(classes_int)
        aos = ref.wants_aos(dt)
        diffs = [0, 1, 2] if cov is None else cov
        with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
            warnings.simplefilter("ignore")
            for m in range(3):
                r = ev.eval_class(gt, dt, classes_int, diffs, m, mo, aos and m == 0)
                for k in ("recall", "real_recall", "precision", "orientation"):
                    out["%s/m%d/%s" % (name, m, k)] = r[k]
            detail = {}
            res, ret, _ = ev.get_official_eval_result(gt, dt, classes, coverage_rates=cov, PR_detail_dict=detail)
        assert np.array_equal(detail["3d"], out["%s/m2/precision" % name], equal_nan=True)
        meta[name] = {"result": res, "ret_dict": {k: float(v) for k, v in ret.items()}, "compute_aos": bool(aos),
                      "frames": len(gt), "n_gt": int(sum(len(a["name"]) for a in gt)), "n_dt": int(sum(len(a["name"]) for a in dt))}
        print(res)
    # the annotation builder: the reference's two box_utils functions on seeded lidar boxes
    ref_env.install(oracle_spconv)
    from btcdet.utils import box_utils, calibration_kitti
    for seed, shape in ((1, (375, 1242)), (2, (370, 1224))):
        c = ref.make_calib(seed)
        calib = calibration_kitti.Calibration({"P2": c["P2"], "R0": c["R0"], "Tr_velo2cam": c["V2C"]})
        boxes = ref.make_lidar_boxes(seed, 40)
        cam = box_utils.boxes3d_lidar_to_kitti_camera(boxes.copy(), calib)
        img = box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=np.array(shape))
        out["builder/%d/camera" % seed], out["builder/%d/image" % seed] = cam, img
        meta["builder/%d" % seed] = {"image_shape": list(shape)}
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "kitti_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
