"""Seeded inputs of the fine-tuning dataset tests (robust_cvd_amd/csrc/cvd_batch.h, robust_cvd_amd/video_dataset.py, DESIGN.md
§3.14): a five-frame dataset directory written with robust_cvd_amd.dataset_io, the replay object that answers the calls
VideoDataset.update_poses makes on a DepthVideo, and the list of recorded batches.  tests/golden/reference_py/make_dataset_golden.py
runs the reference's own VideoDataset on exactly these; the tests regenerate them from the seed.

The smallest shapes at which the batch kernel can still go wrong: 5 x 6 = 30 pixels (no multiple of 4: the element-wise path, planes
that are not 16-byte aligned) and 4 x 8 = 32 pixels (the 16-byte path); N = 2 and N = 6; samples that touch frame 0 and frame 4
(dummy neighbours) and fully interior ones.  Values are small multiples of powers of two, so the fixture compresses.
"""
import json
import os
import types

import numpy as np

from robust_cvd_amd import dataset_io
from robust_cvd_amd.ctypes_types import DepthXformType, SpatialXformType, ValueXformType, XformType

F = 5
FRAMES = list(range(F))
MIN_MASK_RATIO = 0.3
SHAPES = {"odd": (5, 6), "vec": (4, 8)}
# fourteen directed pairs over the five frames, every (k, k +- 1) among them
UNDIRECTED = [(0, 1), (1, 2), (2, 3), (3, 4), (0, 2), (1, 3), (0, 4)]
DIRECTED = [p for a, b in UNDIRECTED for p in ((a, b), (b, a))]
# flow_list.json: (1, 3) passes in one direction only and survives; (0, 4) fails in both and goes; (1, 7) names a frame outside
SCORES = {p: 0.8 for p in DIRECTED}
SCORES.update({(3, 1): 0.1, (0, 4): 0.2, (4, 0): 0.25})
FLOW_LIST = [["frame0", "frame1", "score"]] + [[a, b, SCORES[(a, b)]] for a, b in DIRECTED] + [[1, 7, 0.9], [7, 1, 0.9]]
PAIRS_WITH_LIST = [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3], [3, 4]]           # sorted one-way pairs that survive the list
PAIRS_WITHOUT_LIST = sorted([a, b] for a, b in UNDIRECTED)                   # the directory listing keeps all seven

# name: (shape, temporal, recon, depth transform, flow_list.json present)
CONFIGS = {
    "colmap_odd": ("odd", False, "colmap", None, True),      # N = 2, cameras from a meta file, no update_poses: no scales, no warp
    "grid_vec": ("vec", True, "i3d", "Grid", True),          # N = 6, scale maps and warps
    "grid_odd": ("odd", True, "i3d", "Grid", True),
    "global_vec": ("vec", True, "i3d", "Global", True),      # scales (B, N, 1, 1)
    "nolist_vec": ("vec", False, "colmap", None, False),     # pairs from the directory listing
}


def pairs_of(config):
    return PAIRS_WITH_LIST if CONFIGS[config][4] else PAIRS_WITHOUT_LIST


def batches_of(config):
    """Sample-index lists of the recorded batches: B = 3 over every sample in order (the last one short for seven samples), B = 1
    of the first and the last sample, and one batch that holds a sample twice."""
    S = len(pairs_of(config))
    return [list(range(i, min(i + 3, S))) for i in range(0, S, 3)] + [[0], [S - 1], [2, 0, 2]]


def batch_key(config, pairs):
    """Fixture key of a batch: by its pairs, not by position (the reference's sample order is the iteration order of a set)."""
    return config + "/" + "+".join(f"{a}_{b}" for a, b in pairs)


def make_inputs(config):
    """Everything on disk and in the replay object, from the seed: colors [F, H, W, 3] BGR as the raw files hold them, flows
    {(a, b): [H, W, 2]}, masks {(a, b): [H, W] u8 from {0, 1, 7, 255}}, disparity [F, H, W] of the initial depth, and the pose
    state (right, up, backward, position [F, 3] f32, hfov, vfov [F] f32, param_map [F, H, W] f64, global_scale [F] f64, warp
    [F, H, W, 2] f32)."""
    shape, _temporal, _recon, _depth, _list = CONFIGS[config]
    H, W = SHAPES[shape]
    rng = np.random.default_rng(20240 + sorted(CONFIGS).index(config))
    f32 = np.float32
    inp = {"H": H, "W": W}
    inp["colors"] = (rng.integers(0, 256, (F, H, W, 3)) / 256.0).astype(f32)
    inp["flows"] = {p: (rng.integers(-32, 33, (H, W, 2)) / 4.0).astype(f32) for p in DIRECTED}
    inp["masks"] = {p: rng.choice(np.array([0, 1, 7, 255], np.uint8), (H, W)) for p in DIRECTED}
    inp["disparity"] = (0.25 + rng.integers(0, 64, (F, H, W)) / 32.0).astype(f32)
    for k in ("right", "up", "backward", "position"):
        inp[k] = (rng.integers(-512, 513, (F, 3)) / 256.0).astype(f32)
    inp["hfov"] = (0.6 + rng.integers(0, 64, F) / 128.0).astype(f32)
    inp["vfov"] = (0.4 + rng.integers(0, 64, F) / 128.0).astype(f32)
    inp["param_map"] = 0.5 + rng.integers(0, 256, (F, H, W)) / 256.0
    inp["global_scale"] = 0.5 + rng.integers(0, 256, F) / 256.0
    inp["warp"] = (rng.integers(-64, 65, (F, H, W, 2)) / 1024.0).astype(f32)
    # the cameras of a meta file (the colmap configurations)
    inp["meta_extrinsics"] = (rng.integers(-512, 513, (F, 3, 4)) / 256.0).astype(f32)
    inp["meta_intrinsics"] = (rng.integers(1, 512, (F, 4)) / 4.0).astype(f32)
    return inp


def write_dataset(config, base_dir, inp=None, initial_depth=False):
    """The dataset directory of a configuration; returns (path, meta file or None, initial depth directory or None)."""
    inp = make_inputs(config) if inp is None else inp
    _shape, _temporal, recon, _depth, with_list = CONFIGS[config]
    os.makedirs(base_dir, exist_ok=True)
    dataset_io.write_flow_inputs(base_dir, DIRECTED, [inp["flows"][p] for p in DIRECTED], [inp["masks"][p] for p in DIRECTED],
                                 inp["colors"])
    if with_list:
        with open(os.path.join(base_dir, "flow_list.json"), "w") as f:
            json.dump(FLOW_LIST, f)
    meta = None
    if recon == "colmap":
        meta = os.path.join(base_dir, "metadata.npz")
        np.savez(meta, extrinsics=inp["meta_extrinsics"], intrinsics=inp["meta_intrinsics"])
    depth_dir = None
    if initial_depth:
        depth_dir = os.path.join(base_dir, "depth_initial", "depth")
        os.makedirs(depth_dir, exist_ok=True)
        for i in range(F):
            dataset_io.write_raw_image(os.path.join(depth_dir, f"frame_{i:06d}.raw"), inp["disparity"][i])
    return base_dir, meta, depth_dir


def stub_lib_python():
    """The four names the reference's loaders/video_dataset.py imports from lib_python, as this package's enums (their members
    carry the reference's names and values)."""
    m = types.ModuleType("lib_python")
    m.DepthVideo = object
    m.ValueXformType, m.DepthXformType, m.SpatialXformType, m.XformType = ValueXformType, DepthXformType, SpatialXformType, XformType
    return m


class Replay:
    """The calls VideoDataset.update_poses makes on a lib_python.DepthVideo (reference loaders/video_dataset.py:159-214), answered
    from the seeded pose state.  The maps are seeded arrays, not spline evaluations: the batch path only moves them."""

    def __init__(self, config, inp=None):
        self.config = config
        self.inp = make_inputs(config) if inp is None else inp
        self.depth = CONFIGS[config][3]

    def numFrames(self):
        return F

    def numDepthStreams(self):
        return 1

    def depthStream(self, i):
        assert i == 0
        return self

    def width(self):
        return self.inp["W"]

    def height(self):
        return self.inp["H"]

    def frame(self, i):
        inp = self.inp
        ext = types.SimpleNamespace(right=lambda: inp["right"][i].tolist(), up=lambda: inp["up"][i].tolist(),
                                    backward=lambda: inp["backward"][i].tolist(), position=inp["position"][i].tolist())
        intr = types.SimpleNamespace(hFov=float(inp["hfov"][i]), vFov=float(inp["vfov"][i]))
        ddesc = types.SimpleNamespace(type=XformType.Depth, valueXform=ValueXformType.Scale, depthType=DepthXformType[self.depth],
                                      gridSize=[2, 2, 2], cubicInterpolation=False, depthMinMax=[0.5, 2.0])   # (depth-wise: the host path)
        dx = types.SimpleNamespace(desc=lambda: ddesc, params=lambda: [float(inp["global_scale"][i])],
                                   paramMap=lambda f: inp["param_map"][i])
        # (a type update_poses accepts; the warp itself is the seeded array)
        sdesc = types.SimpleNamespace(type=XformType.Spatial, spatialType=SpatialXformType.BilinearGrid, gridSize=[2, 2, 0])
        sx = types.SimpleNamespace(desc=lambda: sdesc, params=lambda: [], warp=lambda h, w: inp["warp"][i])
        return types.SimpleNamespace(extrinsics=ext, intrinsics=intr, depthXform=lambda: dx, spatialXform=lambda: sx)
