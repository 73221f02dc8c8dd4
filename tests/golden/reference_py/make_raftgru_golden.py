#!/usr/bin/env python3
"""Mint tests/golden/reference_py/raftgru_golden.npz: the reference's SepConvGRU (raft/core/update.py:37-75, f32, CPU) with the
weights of the seeded cases of tests/raftgru_cases.py loaded.  Runs in the build container only (needs the reference and torch;
no GPU):

    python tests/golden/reference_py/make_raftgru_golden.py

Per case `<name>/...`: input_sha256 (digest of the rebuilt inputs, so that a drifted generator is noticed), samples (up to 64 flat
pixel indices: the four corners of image 0 and the last pixel among them), out [len(samples), 128] f32 = the reference's output at
those pixels, delta = max |reference f32 - float64 restatement| over ALL pixels, scale = max |restatement|.  Inputs are not stored;
the file holds recorded results only.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import raftgru_cases as gc  # noqa: E402
from tests import raftgru_reference as gr  # noqa: E402


def main():
    ref = gr.load_reference()
    assert ref is not None, "the reference and torch are needed to mint this file"
    out = {}
    for name in gc.CASES:
        case = gc.make_case(name)
        out32 = gr.reference_output(ref, case)
        out64 = gr.sepconv_gru(case["h"], case["x"], case["weights"], case["biases"])
        assert np.isfinite(out32).all() and np.isfinite(out64).all()
        delta, scale = float(np.abs(out32 - out64).max()), float(np.abs(out64).max())
        print(f"{name}: out {out32.shape}, {len(case['samples'])} pixels stored, delta {delta:.3e} at scale {scale:.3f}")
        out[name + "/input_sha256"] = np.frombuffer(gc.input_digest(case).encode(), np.uint8)
        out[name + "/samples"] = case["samples"]
        out[name + "/out"] = gc.sample_view(case, out32)
        out[name + "/delta"], out[name + "/scale"] = np.float64(delta), np.float64(scale)
    np.savez_compressed(gr.GOLDEN, **out)
    print("wrote", gr.GOLDEN, os.path.getsize(gr.GOLDEN), "bytes")
    assert os.path.getsize(gr.GOLDEN) < 1_000_000


if __name__ == "__main__":
    main()
