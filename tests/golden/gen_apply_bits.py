"""Writes tests/golden/apply_bits.json: per case of tests/test_hip_apply_bits.py the SHA-1 of its inputs and of the result bytes that
conv_apply_b / conv_apply_s give for it.  Run on the GPU, with the kernels whose bits are to be pinned:

    python tests/golden/gen_apply_bits.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p_ in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import test_hip_apply_bits as t  # noqa: E402

out = {}
for spec in t.CASES:
    h_in, h_out = t.run_case(spec)
    out[spec["name"]] = {"inputs": h_in, "result": h_out}
    print(spec["name"], h_in[:12], h_out[:12])
with open(sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN, "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
