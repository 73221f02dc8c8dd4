#!/usr/bin/env python3
"""Mint tests/golden/reference_py/spatial_golden.npz: the REAL DisparitySmoothLoss.forward, ContrastLoss.forward and
JointLoss.__call__ of the reference (loss/disparity_smooth_loss.py, loss/contrast_loss.py, loss/joint_loss.py) with torch autograd
on the CPU, on the seeded cases of tests/spatial_cases.py.

    python tests/golden/reference_py/make_spatial_golden.py

Needs the reference checkout (tests/reference_residuals._reference_modules puts it on the path and stubs cv2).  Recorded per
combination of (case, lambdas, sigma, threshold), float64: `total`, the per-sample `smooth` [B], `contrast`, the gradient table
`grad` [F, H, W], and the reference's own f32 run against its f64 run -- `delta_total` (relative difference of the totals) and
`delta_grad` (max |g32 - g64| / max |g64|), the yardstick of the f32 kernels' test.  Per case the sha256 digest of the inputs.

One joint record, `joint/...`: JointLoss on the case spatial_cases.JOINT_CASE of tests/sceneflow_cases.py (B = 2, N = 6 -- the
reference's ConsistencyLoss accepts the six-frame layout: its loop over the two flow directions reads frames 0 and 1) with
recon = "colmap" and the options spatial_cases.JOINT_OPTIONS: the parameter, consistency, scene-flow and both spatial terms on.
It holds the total (summed by the reference in float32), every entry of batch_losses, the contrast term, the depth gradient and
the gradients of the two parameter tensors.

Only recorded results are written; how the reference is driven is tests/spatial_reference.reference_run / joint_reference_run.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import sceneflow_cases as sfc  # noqa: E402
from tests import spatial_cases as sc  # noqa: E402
from tests import spatial_reference as sr  # noqa: E402


def main():
    out = {}
    for name in sc.CASES:
        case = sc.make_case(name)
        kd, kD, gap, share = sr.check_conditions(case, sc.THRESHOLDS)
        # (a seed that fails: choose another seed, not another bar)
        assert kd >= sr.KINK_DISTANCE and kD >= sr.KINK_DISTANCE and gap >= sr.THRESHOLD_DISTANCE, (name, kd, kD, gap)
        assert name == "tiny" or all(sr.MASK_SHARE[0] <= v <= sr.MASK_SHARE[1] for v in share.values()), (name, share)
        out[f"{name}/digest"] = np.frombuffer(sc.digest(case).encode(), np.uint8)
        print(f"{name}: kinks {kd:.2e} {kD:.2e}  threshold gap {gap:.2e}  mask share {share}")
    for combo in sc.COMBOS:
        case = sc.make_case(combo[0])
        key = sc.combo_key(combo)
        t64, s64, c64, g64 = sr.reference_run(case, *combo[1:], "float64")
        t32, _s32, _c32, g32 = sr.reference_run(case, *combo[1:], "float32")
        assert np.isfinite(t64) and np.isfinite(g64).all() and np.isfinite(g32).all()
        out[f"{key}/total"] = np.float64(t64)
        out[f"{key}/smooth"] = s64
        out[f"{key}/contrast"] = np.float64(c64)
        out[f"{key}/grad"] = g64
        out[f"{key}/delta_total"] = np.float64(abs(t32 - t64) / abs(t64))
        out[f"{key}/delta_grad"] = np.float64(np.abs(g32 - g64).max() / np.abs(g64).max())
        print(f"{key}: total {t64:.12g}  delta_total {out[f'{key}/delta_total']:.2e}  delta_grad {out[f'{key}/delta_grad']:.2e}")
    case = sfc.make_case(sc.JOINT_CASE)
    total, batch, contrast, grad, pgrads = sr.joint_reference_run(case, sc.joint_inputs(case), sc.JOINT_OPTIONS)
    assert np.isfinite(total) and np.isfinite(grad).all()
    out["joint/digest"] = np.frombuffer(sfc.digest(case).encode(), np.uint8)
    out["joint/total"] = np.float64(total)
    out["joint/contrast"] = np.float64(contrast)
    out["joint/grad"] = grad
    for k, v in batch.items():
        out[f"joint/batch/{k}"] = v
    for i, g in enumerate(pgrads):
        out[f"joint/parameter_grad/{i}"] = g
    print("joint: total", total, {k: v.ravel()[:2] for k, v in batch.items()}, "contrast", contrast)
    np.savez_compressed(sr.GOLDEN, **out)
    size = os.path.getsize(sr.GOLDEN)
    assert size < (1 << 20), size
    print("wrote", sr.GOLDEN, size, "bytes")


if __name__ == "__main__":
    main()
