#!/usr/bin/env python3
"""Mint tests/golden/reference_py/flowmask_golden.npz: the reference's flow consistency masks (utils/consistency.py:
consistent_flow_masks) and its own f32 error maps (its `sample` + `sse`) on the seeded cases of tests/flowmask_cases.py.  Runs in
the build container only (needs the reference and torch; no GPU, no cv2):

    python tests/golden/reference_py/make_flowmask_golden.py

Per case `<name>/...`: input_sha256 (digest of the rebuilt inputs, so that a drifted generator is noticed), shape [U, 2, H, W],
mask_bits (np.packbits of the reference's masks of every unordered pair, both directions), err_pairs (indices of the unordered
pairs whose error maps are stored: four per case, the longest baseline among them), errors [len(err_pairs), 2, H, W, 2] f32
(ef, ec) -- or errors_case, the name of the case with the same images whose errors apply --, delta = max |e_ref32 - e_f64| over
every direction's finite errors < 10 and delta_rel = max relative difference over the others (e_f64: tests/flowmask_reference.py),
undecided_bits (packbits of the pixels with |e_ref32 - threshold| <= 8 delta for either error), undecided_share, kept_share.
The script asserts the cap of 0.1 % undecided pixels per case and that the f64 restatement reproduces every decided pixel.
Inputs are not stored; the file holds recorded results only.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import flowmask_cases as fc  # noqa: E402
from tests import flowmask_reference as fr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_py", "flowmask_golden.npz")


def main():
    cons = fr.load_reference_consistency()
    assert cons is not None, "the reference and torch are needed to mint this file"
    out, stored = {}, {}
    for name in fc.CASES:
        case = fc.make_case(name)
        color, pairs, fab, fba = case["color"], case["pairs"], case["flow_ab"], case["flow_ba"]
        ft, ct = case["flow_thresh"], case["color_thresh"]
        U, H, W = fab.shape[:3]
        masks = np.zeros((U, 2, H, W), bool)
        err = np.zeros((U, 2, H, W, 2), np.float32)
        for p, (a, b) in enumerate(pairs.tolist()):
            masks[p], err[p] = fr.reference_pair(cons, fab[p], fba[p], color[a], color[b], ft, ct)
        mab, mba, _kept, e64 = fr.batch(color, pairs, fab, fba, ft, ct)
        delta, delta_rel = fr.deltas(err, e64)
        und = fr.undecided(err, delta, ft, ct, color.shape[-1])
        share = float(und.mean())
        mine = np.stack([mab, mba], axis=1) > 0
        wrong = int(((mine != masks) & ~und).sum())
        print(f"{name}: {U} pairs {W}x{H}, delta {delta:.3e}, delta_rel {delta_rel:.3e}, undecided {int(und.sum())} of {und.size} "
              f"({100 * share:.4f} %), kept {100 * masks.mean():.1f} %, f64 restatement differs on {wrong} decided pixels")
        assert share <= fr.MAX_UNDECIDED, "more than 0.1 % undecided pixels: change the case's inputs, not the cap"
        assert wrong == 0
        ep = fc.error_pairs(pairs) if U > 1 else np.array([0], np.int64)
        images = fc.input_digest({**case, "flow_thresh": 0.0, "color_thresh": 0.0})
        out[name + "/input_sha256"] = np.frombuffer(fc.input_digest(case).encode(), np.uint8)
        out[name + "/shape"] = np.array([U, 2, H, W], np.int32)
        out[name + "/mask_bits"] = np.packbits(masks)
        out[name + "/undecided_bits"] = np.packbits(und)
        out[name + "/err_pairs"] = ep
        if images in stored:
            out[name + "/errors_case"] = np.frombuffer(stored[images].encode(), np.uint8)
        else:
            out[name + "/errors"] = err[ep]
            stored[images] = name
        out[name + "/delta"] = np.float64(delta)
        out[name + "/delta_rel"] = np.float64(delta_rel)
        out[name + "/undecided_share"] = np.float64(share)
        out[name + "/kept_share"] = np.float64(masks.mean())
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
    assert os.path.getsize(GOLDEN) < (1 << 20)


if __name__ == "__main__":
    main()
