"""Generates tests/golden/ref_dropin.json: the state_dict keys / shapes / dtypes (and the backbones' num_point_features and sparse_shape)
of the reference's own modules that tests/test_reference_dropin_cpu.py compares this repository's against, built on btcdet_amd.spconv
and the pointnet2 stand-in.  Runs only where the reference tree is there; the test uses the file where it is not.

    python tests/golden/gen_dropin_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p_ in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p_)

import importlib.util  # noqa: E402

import btcdet_amd  # noqa: E402
import test_reference_dropin_cpu as t  # noqa: E402
from btcdet_amd import pointnet2_stack as p2  # noqa: E402

if __name__ == "__main__":
    assert os.path.exists(t.REF) and os.path.exists(t.PN2_ROOT), "the reference tree is not there"
    btcdet_amd.install_as_spconv()
    spec = importlib.util.spec_from_file_location("_ref_spconv_backbone", t.REF)
    ref_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_mod)
    _, p2_mods = t.load_reference_pointnet2(p2)
    out = {name: (t.record_block(m) if name == "post_act_block" else t.record(m)) for name, m in t.reference_modules(ref_mod, p2_mods).items()}
    with open(os.path.join(HERE, "ref_dropin.json"), "w") as f:   # one state_dict entry per line
        f.write("{\n" + ",\n".join("%s: {%s}" % (json.dumps(name), ",\n ".join(
            "%s: [\n  %s]" % (json.dumps(k), ",\n  ".join(json.dumps(e) for e in v)) if k == "state" else "%s: %s" % (json.dumps(k), json.dumps(v))
            for k, v in sorted(rec.items()))) for name, rec in sorted(out.items())) + "\n}\n")
    print("wrote", os.path.join(HERE, "ref_dropin.json"), {k: len(v["state"]) for k, v in out.items()})
