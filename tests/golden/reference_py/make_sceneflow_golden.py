#!/usr/bin/env python3
"""Mint tests/golden/reference_py/sceneflow_golden.npz: the REAL SceneFlowLoss.__call__ of the reference
(loss/scene_flow_loss.py) with torch autograd on the CPU, on the seeded cases of tests/sceneflow_cases.py.

    python tests/golden/reference_py/make_sceneflow_golden.py

Needs the reference checkout (tests/reference_residuals._reference_modules puts it on the path and stubs cv2).  Recorded per
combination of (case, distances, lambdas), float64: `total`, the per-pair `terms` [P, 4] (static, smooth_reproj,
smooth_disparity, smooth_depth_ratio; 0 where the term does not exist), the gradient table `grad` [F, H, W], and the reference's
own f32 run against its f64 run -- `delta_total` (relative difference of the totals) and `delta_grad` (max |g32 - g64| /
max |g64|), the yardstick of the f32 kernels' test.  For one combination (sceneflow_cases.MAPS_COMBO) the six visualisation
`maps` [6, P, 3, H, W].  Per case the sha256 digest of the inputs.  Only recorded results are written; how the reference is
driven is tests/sceneflow_reference.reference_run.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import sceneflow_cases as sc  # noqa: E402
from tests import sceneflow_reference as sr  # noqa: E402


def main():
    out = {}
    for name in sc.CASES:
        case = sc.make_case(name)
        kinks = sr.check_kinks(case)
        assert min(kinks) >= sr.KINK_DISTANCE, (name, kinks)   # (a seed that fails: choose another seed, not another bar)
        out[f"{name}/digest"] = np.frombuffer(sc.digest(case).encode(), np.uint8)
    for combo in sc.COMBOS:
        case = sc.make_case(combo[0])
        key = sc.combo_key(combo)
        t64, terms64, g64, maps64 = sr.reference_run(case, *combo[1:], "float64")
        t32, _terms32, g32, _maps32 = sr.reference_run(case, *combo[1:], "float32")
        assert np.isfinite(t64) and np.isfinite(g64).all() and np.isfinite(g32).all()
        terms = np.zeros((case["P"], 4))
        for q, term in enumerate(sr.TERMS):
            if term in terms64:
                terms[:, q] = terms64[term]
        out[f"{key}/total"] = np.float64(t64)
        out[f"{key}/terms"] = terms
        out[f"{key}/grad"] = g64
        out[f"{key}/delta_total"] = np.float64(abs(t32 - t64) / abs(t64))
        out[f"{key}/delta_grad"] = np.float64(np.abs(g32 - g64).max() / np.abs(g64).max())
        if combo == sc.MAPS_COMBO:
            assert len(maps64) == 6
            out[f"{key}/maps"] = np.stack(maps64, 0)
        print(f"{key}: total {t64:.12g}  delta_total {out[f'{key}/delta_total']:.2e}  delta_grad {out[f'{key}/delta_grad']:.2e}")
    np.savez_compressed(sr.GOLDEN, **out)
    size = os.path.getsize(sr.GOLDEN)
    assert size < (1 << 20), size
    print("wrote", sr.GOLDEN, size, "bytes")


if __name__ == "__main__":
    main()
