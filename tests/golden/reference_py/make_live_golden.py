#!/usr/bin/env python3
"""Mint tests/golden/reference_py/live_golden.npz: what the reference's own Python functions return for the inputs of the
"live" pins, so that those pins run from a clean checkout without the reference next to it.  Needs a checkout of the reference
(its directory as the argument) and torch; no GPU:

    python tests/golden/reference_py/make_live_golden.py <reference checkout>

Keys:
  res/<case>/rows, res/<case>/fd, res/<case>/fd_depth  the central differences of the reference's torch functions
                                      (tests/reference_residuals.py `reference_outputs`) for every 8th constraint from the 4th on --
                                      the rows residual_golden.npz does not keep (it keeps every 8th from the 0th): fd [m, 3, 14] as
                                      float32, fd_depth [m, 3, 2] as float32
  raw/image_<i>/bytes, raw/image_<i>/read  utils/image_io.py's writer on the seeded images of test_reference_raw_images.py, and its
                                      reader on those bytes
  raw/stream_<i>/bytes                the writer on 1 / depth of frame i of the seeded 4-frame depth stream
  reproj/...                          VideoDataset.update_poses + utils/geometry.py on the synthetic generator's TRUE cameras and
                                      scales (tests/reference_reprojection.py's case): extrinsics, intrinsics and every constraint's
                                      reprojected pixel minus its flow target
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from robust_cvd_amd import synth  # noqa: E402
from tests import baseline_configs as bc  # noqa: E402
from tests import reference_reprojection as rr  # noqa: E402
from tests import reference_residuals as rres  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "live_golden.npz")
RAW_SHAPES = ((9, 13), (6, 8, 2), (4, 4, 3))
FD_FIRST, FD_EVERY = 4, 8   # (residual_golden.npz: rows 0, 8, 16, ...)


def raw_inputs():
    """The seeded images and the depth stream the raw-format pin writes (shared with tests/test_reference_raw_images.py)."""
    rng = np.random.default_rng(5)
    images = [rng.standard_normal(shape).astype(np.float32) for shape in RAW_SHAPES]
    return images, synth.make_video(4, 48, 28, seed=89, spacing=8)


def truth_outputs(v):
    """The synthetic generator's TRUE cameras / scales in the form of the optimizer's getters."""
    F, H, W = v.num_frames, v.height, v.width
    R = synth.rodrigues(v.true_w)
    return dict(right=R[:, :, 0], up=R[:, :, 1], backward=R[:, :, 2], position=v.true_t,
                hfov=np.full(F, 2 * np.arctan(v.true_fy * v.aspect)), vfov=np.full(F, 2 * np.arctan(v.true_fy)),
                param_map=np.stack([v.frame_scale[f] * rr.grid_field(v.true_theta[f], W, H) for f in range(F)]),
                params=v.frame_scale[:, None],
                warp=np.zeros((F, H, W, 2), np.float32), source_depth=v.depth, width=np.int32(W), height=np.int32(H),
                depth_desc=np.frombuffer(b"Grid(Scale, Linear, 4, 3, 1)", np.uint8))


def main(reference_dir):
    sys.path.insert(0, os.path.abspath(reference_dir))
    out = {}
    for name in rres.CASES:
        ref = rres.reference_outputs(name)
        rows = np.arange(FD_FIRST, len(ref["fd"]), FD_EVERY)
        out[f"res/{name}/rows"] = rows.astype(np.int32)
        out[f"res/{name}/fd"] = ref["fd"][rows].astype(np.float32)
        out[f"res/{name}/fd_depth"] = ref["fd_depth"][rows].astype(np.float32)
    from utils import image_io  # (importable once reference_outputs has stubbed cv2)
    images, v = raw_inputs()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "img.raw")
        for i, img in enumerate(images):
            image_io.save_raw_float32_image(path, img)
            out[f"raw/image_{i}/bytes"] = np.frombuffer(open(path, "rb").read(), np.uint8)
            out[f"raw/image_{i}/read"] = np.asarray(image_io.load_raw_float32_image(path), np.float32)
        for i in range(v.num_frames):
            image_io.save_raw_float32_image(path, 1.0 / v.depth[i])
            out[f"raw/stream_{i}/bytes"] = np.frombuffer(open(path, "rb").read(), np.uint8)
    spec = importlib.util.spec_from_file_location(
        "make_reprojection_golden", os.path.join(os.path.dirname(rr.GOLDEN), "make_reprojection_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    case = rr.make_case()
    ref = mk.reference_outputs(truth_outputs(case), case)
    out["reproj/input_sha256"] = np.frombuffer(bc.input_digest(case).encode(), np.uint8)
    for k in ("ref_extrinsics", "ref_intrinsics"):
        out["reproj/" + k] = ref[k]
    # the reprojected pixels as their offsets from the flow targets (below 1e-3 px: float16 keeps them to 1e-6 px)
    out["reproj/ref_offset_from_target"] = (ref["ref_reprojected"] - ref["target_pixel"]).astype(np.float16)
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
