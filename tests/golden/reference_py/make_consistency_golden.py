#!/usr/bin/env python3
"""Mint tests/golden/reference_py/consistency_golden.npz: the REAL ConsistencyLoss.__call__ of the reference
(loss/consistency_loss.py) with torch autograd on the CPU, on the seeded cases of tests/consistency_cases.py.

    python tests/golden/reference_py/make_consistency_golden.py

Needs the reference checkout (tests/reference_residuals._reference_modules puts it on the path and stubs cv2).  Recorded per
combination of (case, distance, lambdas), float64: `total`, the per-pair `terms` [P, 3] (reproj, disp, depth ratio; 0 where the
term does not exist), the gradient table `grad` [F, H, W], and the reference's own f32 run against its f64 run -- `delta_total`
(relative difference of the totals) and `delta_grad` (max |g32 - g64| / max |g64|), the yardstick of the f32 kernels' test.  Per
case the sha256 digest of the inputs.  Only recorded results are written; how the reference is driven (and the three things to
know about it) is tests/consistency_reference.reference_run.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import consistency_cases as cc  # noqa: E402
from tests import consistency_reference as cr  # noqa: E402


def main():
    out = {}
    for name in cc.CASES:
        case = cc.make_case(name)
        kinks = cr.check_kinks(case)
        assert min(kinks) >= cr.KINK_DISTANCE, (name, kinks)   # (a seed that fails: choose another seed, not another bar)
        out[f"{name}/digest"] = np.frombuffer(cc.digest(case).encode(), np.uint8)
    for combo in cc.COMBOS:
        case = cc.make_case(combo[0])
        key = cc.combo_key(combo)
        t64, terms64, g64 = cr.reference_run(case, *combo[1:], "float64")
        t32, _terms32, g32 = cr.reference_run(case, *combo[1:], "float32")
        terms = np.zeros((case["P"], 3))
        for q, term in enumerate(cr.TERMS):
            if term in terms64:
                terms[:, q] = terms64[term]
        out[f"{key}/total"] = np.float64(t64)
        out[f"{key}/terms"] = terms
        out[f"{key}/grad"] = g64
        out[f"{key}/delta_total"] = np.float64(abs(t32 - t64) / abs(t64))
        out[f"{key}/delta_grad"] = np.float64(np.abs(g32 - g64).max() / np.abs(g64).max())
        print(f"{key}: total {t64:.12g}  delta_total {out[f'{key}/delta_total']:.2e}  delta_grad {out[f'{key}/delta_grad']:.2e}")
    np.savez_compressed(cr.GOLDEN, **out)
    size = os.path.getsize(cr.GOLDEN)
    assert size < (1 << 20), size
    print("wrote", cr.GOLDEN, size, "bytes")


if __name__ == "__main__":
    main()
