#!/usr/bin/env python3
"""Mint tests/golden/reference_py/dataset_golden.npz: the reference's OWN VideoDataset (loaders/video_dataset.py) and torch's
default collate, on CPU tensors, on the seeded five-frame datasets of tests/dataset_cases.py.

    python tests/golden/reference_py/make_dataset_golden.py <reference checkout>

Per configuration of dataset_cases.CONFIGS the dataset directory is written to a temporary directory with
robust_cvd_amd.dataset_io, the reference's class is constructed on it, update_poses runs on dataset_cases.Replay (seeded cameras,
maps and warps; not for the colmap configurations, which read their cameras from a meta file) and the batches of
dataset_cases.batches_of are collated by torch.utils.data.DataLoader(batch_size=B, shuffle=False, num_workers=0) over the sample
positions that hold the wanted pairs.  Every tensor of every batch is recorded under `<config>/<a>_<b>+<a>_<b>.../<name>`, with
the flat names of robust_cvd_amd.api.dataset_batch_shapes: keyed by the pairs, because the reference's sample order is the
iteration order of a set.  `<config>/flow_indices`: its pair list, sorted.

`cv2` (not installed) is stubbed with imread through Pillow, BGR as OpenCV decodes; `lib_python` is a stub of the four names the
reference imports.  Only what the reference returned is written.
"""
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import dataset_cases as dc  # noqa: E402
from tests import dataset_reference as dr  # noqa: E402


def stub_cv2():
    from PIL import Image
    cv2 = types.ModuleType("cv2")
    cv2.CV_32FC3, cv2.CV_8UC1, cv2.IMREAD_UNCHANGED = 21, 0, -1

    def imread(path, flags=None):
        im = np.asarray(Image.open(path))
        return im[..., ::-1].copy() if im.ndim == 3 else im.copy()
    cv2.imread = imread
    return cv2


def flatten(images, meta):
    """(images, metadata) of the reference as the flat names of api.dataset_batch_shapes"""
    out = {"images": images, "extrinsics": meta["extrinsics"], "intrinsics": meta["intrinsics"],
           "gc_indices": meta["geometry_consistency"]["indices"]}
    for d in range(2):
        out[f"gc_flows{d}"] = meta["geometry_consistency"]["flows"][d]
        out[f"gc_masks{d}"] = meta["geometry_consistency"]["masks"][d]
    if "temporal_smoothness" in meta:
        ts = meta["temporal_smoothness"]
        out["ts_indices"], out["ts_valid"] = ts["indices"], ts["valid"]
        for d in range(4):
            out[f"ts_flows{d}"], out[f"ts_masks{d}"] = ts["flows"][d], ts["masks"][d]
    for k in ("scales", "warp"):
        if k in meta:
            out[k] = meta[k]
    return {k: v.numpy() for k, v in out.items()}


def main(reference):
    import torch
    sys.modules.setdefault("cv2", stub_cv2())
    sys.modules.setdefault("lib_python", dc.stub_lib_python())
    sys.path.insert(0, reference)
    from loaders.video_dataset import VideoDataset   # the reference's class
    out = {}
    for config, (_shape, temporal, recon, _depth, _list) in dc.CONFIGS.items():
        inp = dc.make_inputs(config)
        with tempfile.TemporaryDirectory() as tmp:
            path, meta, _ = dc.write_dataset(config, os.path.join(tmp, config), inp)
            ds = VideoDataset(path, dc.FRAMES, dc.MIN_MASK_RATIO, temporal, meta, recon)
            if recon != "colmap":
                ds.update_poses(dc.Replay(config, inp))
            order = [list(p) for p in ds.flow_indices]
            pairs = dc.pairs_of(config)
            assert sorted(order) == pairs, (config, order)
            out[f"{config}/flow_indices"] = np.array(sorted(order), np.int64)
            for idx in dc.batches_of(config):
                want = [pairs[i] for i in idx]
                loader = torch.utils.data.DataLoader(ds, batch_size=len(idx), shuffle=False, num_workers=0,
                                                     sampler=[order.index(p) for p in want])
                (images, metadata), = list(loader)
                flat = flatten(images, metadata)
                assert flat["gc_indices"].tolist() == want
                for name, a in flat.items():
                    assert a.dtype == (np.int64 if name.endswith("indices") else np.float32), (name, a.dtype)
                    out[f"{dc.batch_key(config, want)}/{name}"] = a
                # the restatement the GPU tests compare with reproduces the reference bit for bit
                mine = dr.batch(config, inp, want)
                assert sorted(mine) == sorted(flat), (sorted(mine), sorted(flat))
                for name, a in flat.items():
                    assert mine[name].dtype == a.dtype and mine[name].shape == a.shape and np.array_equal(mine[name], a), (config, name)
            print(f"{config}: {len(order)} samples in the reference's order {order}, {len(dc.batches_of(config))} batches")
    np.savez_compressed(dr.GOLDEN, **out)
    size = os.path.getsize(dr.GOLDEN)
    print(f"{dr.GOLDEN}: {size} bytes, {len(out)} arrays")
    assert size < 1 << 20


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
