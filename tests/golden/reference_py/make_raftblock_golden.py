#!/usr/bin/env python3
"""Mint tests/golden/reference_py/raftblock_golden.npz: the reference's BasicUpdateBlock (raft/core/update.py:133-156, f32, CPU)
with the weights of the seeded block cases of tests/raftblock_cases.py loaded, and its layers' own function (nn.Conv2d's
F.conv2d, F.relu, the factor 0.25) on the single-convolution cases.  Runs in the build container only (needs the reference and
torch; no GPU):

    python tests/golden/reference_py/make_raftblock_golden.py

Per block case `block/<name>/...`: input_sha256 (digest of the rebuilt inputs, so that a drifted generator is noticed), samples
(flat pixel indices: the four corners of image 0 and the last pixel among them) and per output o in (net, mask, delta_flow):
o [len(samples), channels] f32 = the reference's output at those pixels, o_delta = max |reference f32 - float64 restatement| over
ALL pixels, o_scale = max |restatement|.  Per single convolution `conv/<name>/...`: the same with one output `out`.
`state_dict_keys`: the keys of the reference module's state dict, in its order.  Inputs are not stored; the file holds recorded
results only.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import raftblock_cases as bc  # noqa: E402
from tests import raftblock_reference as br  # noqa: E402


def record(out, prefix, case, name, got32, want64):
    assert np.isfinite(got32).all() and np.isfinite(want64).all() and got32.shape == want64.shape
    delta, scale = float(np.abs(got32 - want64).max()), float(np.abs(want64).max())
    print(f"{prefix}: {name} {got32.shape}, {len(case['samples'])} pixels stored, delta {delta:.3e} at scale {scale:.3f}")
    out[f"{prefix}/{name}"] = bc.sample_view(case, got32)
    out[f"{prefix}/{name}_delta"], out[f"{prefix}/{name}_scale"] = np.float64(delta), np.float64(scale)


def main():
    ref = br.load_reference()
    assert ref is not None, "the reference and torch are needed to mint this file"
    out = {"state_dict_keys": np.array(list(ref(br.Args(), hidden_dim=128, input_dim=128).state_dict().keys()))}
    for name in bc.CONV_CASES:
        case = bc.make_conv_case(name)
        prefix = "conv/" + name
        out[prefix + "/input_sha256"] = np.frombuffer(bc.input_digest(case).encode(), np.uint8)
        out[prefix + "/samples"] = case["samples"]
        record(out, prefix, case, "out", br.reference_conv_output(case), br.conv_case(case))
    for name in bc.BLOCK_CASES:
        case = bc.make_block_case(name)
        prefix = "block/" + name
        out[prefix + "/input_sha256"] = np.frombuffer(bc.input_digest(case).encode(), np.uint8)
        out[prefix + "/samples"] = case["samples"]
        for o, got32, want64 in zip(bc.OUTPUTS, br.reference_block_output(ref, case), br.block_case(case)):
            record(out, prefix, case, o, got32, want64)
    np.savez_compressed(br.GOLDEN, **out)
    print("wrote", br.GOLDEN, os.path.getsize(br.GOLDEN), "bytes")
    assert os.path.getsize(br.GOLDEN) < 1_000_000


if __name__ == "__main__":
    main()
