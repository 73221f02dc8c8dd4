#!/usr/bin/env python3
"""Mint tests/golden/reference_py/raftops_golden.npz: the reference's CorrBlock (raft/core/corr.py) and RAFT.upsample_flow
(raft/core/raft.py:49-60) on the seeded cases of tests/raftops_cases.py, on the CPU.  Runs in the build container only (needs the
reference, torch and scipy, which raft/core/utils/utils.py imports; no GPU, no cv2):

    python tests/golden/reference_py/make_raftops_golden.py

Per correlation case `<name>/...`: input_sha256 (digest of the rebuilt inputs, so that a drifted generator is noticed), queries
(the stored queries: all of square16, 256 seeded ones of the other two -- the planted cells and the last query among them),
lookup [len(queries), L n^2] f32 = the reference's output at those queries, pyr<l> [len(queries), h_l, w_l] f32 = the reference's
pooled levels l >= 1 of those queries (level 0 is raw / sqrt(dim), which the tests form themselves and compare bit for bit),
delta_lookup / scale_lookup and delta_pyr / scale_pyr = max |reference f32 - float64 restatement| over ALL queries and the
largest |value| of the restatement.  Per upsampling case: input_sha256, out (the reference's f32 result), delta, scale.  The script
asserts that the reference gives exact zeros at the planted outside / huge coordinates and that level 0 is the f32 quotient.
Inputs are not stored; the file holds recorded results only.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import raftops_cases as rc  # noqa: E402
from tests import raftops_reference as rr  # noqa: E402


def main():
    ref = rr.load_reference()
    assert ref is not None, "the reference and torch are needed to mint this file"
    out = {}
    for name in rc.CORR:
        case = rc.make_corr_case(name)
        pyr32, look32 = rr.reference_outputs(ref, case)
        assert np.array_equal(pyr32[0], rr.level0_f32(case["raw"], case["dim"])), "level 0 is not raw / sqrt(dim) bit for bit"
        pyr64 = rr.pyramid(case["raw"], case["dim"], case["levels"])
        look64 = rr.lookup(pyr64, case["coords"], case["r"])
        q = case["queries"]
        flat = look32.transpose(0, 2, 3, 1).reshape(len(case["raw"]), -1)
        assert not flat[list(rc.ZERO_CELLS)].any(), "the reference is not zero at the planted outside coordinates"
        d_look, s_look = float(np.abs(look32 - look64).max()), float(np.abs(look64).max())
        d_pyr = max(float(np.abs(a - b).max()) for a, b in zip(pyr32[1:], pyr64[1:]))
        s_pyr = max(float(np.abs(b).max()) for b in pyr64[1:])
        print(f"{name}: {len(case['raw'])} queries, {len(q)} stored; lookup delta {d_look:.3e} at scale {s_look:.3f}, "
              f"pooled levels delta {d_pyr:.3e} at scale {s_pyr:.3f}")
        out[name + "/input_sha256"] = np.frombuffer(rc.input_digest(case).encode(), np.uint8)
        out[name + "/queries"] = q
        out[name + "/lookup"] = rc.query_view(case, look32)
        for l in range(1, case["levels"]):
            out[f"{name}/pyr{l}"] = pyr32[l][q]
        out[name + "/delta_lookup"], out[name + "/scale_lookup"] = np.float64(d_look), np.float64(s_look)
        out[name + "/delta_pyr"], out[name + "/scale_pyr"] = np.float64(d_pyr), np.float64(s_pyr)
    for name in rc.UPSAMPLE:
        case = rc.make_upsample_case(name)
        up32 = rr.reference_upsample(ref, case)
        up64 = rr.upsample(case["flow"], case["mask"])
        delta, scale = float(np.abs(up32 - up64).max()), float(np.abs(up64).max())
        print(f"{name}: out {up32.shape}, delta {delta:.3e} at scale {scale:.3f}")
        out[name + "/input_sha256"] = np.frombuffer(rc.input_digest(case).encode(), np.uint8)
        out[name + "/out"] = up32
        out[name + "/delta"], out[name + "/scale"] = np.float64(delta), np.float64(scale)
    np.savez_compressed(rr.GOLDEN, **out)
    print("wrote", rr.GOLDEN, os.path.getsize(rr.GOLDEN), "bytes")
    assert os.path.getsize(rr.GOLDEN) < 1_000_000


if __name__ == "__main__":
    main()
