"""BASELINE.json configs[0..2] at their REAL sizes, as one recipe shared by the fixture minting script
(tests/golden/make_solutions.py: CPU oracle, block-sparse exact Cholesky) and the GPU parity tests
(tests/test_gpu_baseline_configs.py: HIP path with the default = benchmarked solver options).

  config0: 30 frames 192x112, fixed intrinsics, global-scale-only deformation (one LM solve)
  config1: 100 frames 384x224, 4x4 bicubic spline grid (one LM solve from the normalised global scale)
  config2: 300 frames 384x224, hierarchical2 flow list (1766 directed pairs), the default pipeline of
           pose_optimization.py: normalizeDepth + coarse-to-fine Global -> 6x4 -> 12x7 -> 17x10
  config4 / config4_huber: 1000 frames 640x384, 5958 directed pairs (10.4 M constraints), default pipeline ending at the 16x12
           grid, Cauchy 0.5 resp. Huber 0.5 -- the problem `bench.py --config 4` times; sparsified coarse level on the device
  config2_4k: config2 with the "~4k pairs" flow list of BASELINE.json's north_star (extra_offsets = 6: 4140 directed pairs,
           2.40 M constraints) -- the problem bench.py times; its solves run the DENSE coarse level on the device
"""
import hashlib
import os

import numpy as np

from robust_cvd_amd import synth
from robust_cvd_amd.ctypes_types import IntrinsicsOptimization, OptParams, XformDesc

SOLUTIONS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solutions")

CONFIGS = {
    # name: (frames, width, height, seed, extra pair level)
    "config0": dict(frames=30, width=192, height=112, seed=1235),
    "config1": dict(frames=100, width=384, height=224, seed=1236),
    "config2": dict(frames=300, width=384, height=224, seed=1237),
    # the BENCHMARKED problem (bench.py default): the same video with the flow list densified to 4140 directed pairs
    "config2_4k": dict(frames=300, width=384, height=224, seed=1237, extra_offsets=6),
    # BASELINE.json configs[4] on one GPU (bench.py --config 4 [--robust huber]): 1000 frames 640x384, 5958 directed pairs,
    # 10.4 M constraints, default pipeline with the 16x12 grid as its last level (B = 199); the sparsified coarse level
    "config4": dict(frames=1000, width=640, height=384, seed=1237, ctf=(16, 12)),
    "config4_huber": dict(frames=1000, width=640, height=384, seed=1237, ctf=(16, 12), robust=1),
    # DENSE mode at real resolution (matchSeparation = 0: every masked pixel of every directed pair, 12.8 M constraints): the
    # HIP path reads the flow / mask images, the oracle the equivalent constraint list
    "dense30": dict(frames=30, width=384, height=224, seed=1240, dense=True),
    # OFF the tuning set (VERDICT r4 Next #8: the defaults of cvd_solver_options were chosen on seed 1237 at 300 frames): another
    # seed at 150 frames, and a third seed with 1 px flow noise and 5 % gross outliers -- default options against the oracle
    "sweep150": dict(frames=150, width=384, height=224, seed=1, extra_offsets=6),
    "sweep150_noisy": dict(frames=150, width=384, height=224, seed=3, extra_offsets=6, flow_noise_px=1.0, outlier_fraction=0.05),
}


def make_video(name):
    c = CONFIGS[name]
    return synth.make_video(c["frames"], c["width"], c["height"], seed=c["seed"], extra_offsets=c.get("extra_offsets", 1),
                            spacing=(1e9 if c.get("dense") else 12.5),  # (dense: the sampled list is not used)
                            flow_noise_px=c.get("flow_noise_px", 0.25), outlier_fraction=c.get("outlier_fraction", 0.0))


def input_digest(video):
    h = hashlib.sha256()
    for a in (video.depth, video.pairs, video.offsets, video.loc):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def dense_inputs(video):
    """Flow / mask images of every directed pair and the constraint list the reference's compute() makes of them with
    matchSeparation = 0 (cached on the video object)."""
    if getattr(video, "dense_flow", None) is None:
        video.dense_flow, video.dense_mask = synth.make_dense_flows(video)
        video.dense_offsets, video.dense_loc = synth.dense_constraints_from_flows(video, video.dense_flow, video.dense_mask)
    return video.dense_flow, video.dense_mask, video.dense_offsets, video.dense_loc


def load_dense(binding, video, focal_long):
    """Dense mode hand-over: images for the product Solver (cvd_set_pair_flows), the equivalent list for the Oracle."""
    flow, mask, off, loc = dense_inputs(video)
    binding.set_video(video.num_frames, video.width, video.height, video.aspect, video.inv_aspect)
    binding.set_depth_all(video.depth)
    if hasattr(binding, "set_pair_flows"):
        binding.set_pair_flows(video.pairs, flow, mask)
    else:
        binding.set_pair_constraints(video.pairs, off, loc, None)
    binding.reset_poses(focal_long)


def params_for(name, threads=8):
    p = OptParams.defaults()
    p.num_threads = threads
    if name == "config0":
        p.intr_opt = IntrinsicsOptimization.Fixed
        p.coarse_to_fine = 0
        p.num_steps = 1
    elif name == "config1":
        p.coarse_to_fine = 0
        p.num_steps = 1
    if "ctf" in CONFIGS[name]:
        p.ctf_long, p.ctf_short = CONFIGS[name]["ctf"]
    return p


def run(binding, name, video, threads=8):
    """The solve of one config on `binding` (product Solver or test Oracle); returns the end state."""
    p = params_for(name, threads)
    if CONFIGS[name].get("robust"):
        binding.set_robust_loss(CONFIGS[name]["robust"])  # (1 = Huber: the stress variant BASELINE.json configs[4] names)
    if CONFIGS[name].get("dense"):
        load_dense(binding, video, p.focal_long)
    else:
        synth.load_into(binding, video, p.focal_long)
    binding.reset_depth_xforms(XformDesc.global_depth())
    binding.reset_spatial_xforms(XformDesc.spatial())
    binding.normalize_depth(p)
    if name == "config1":
        binding.grid_xform_split(XformDesc.grid_depth(4, 4, cubic=True))
    binding.pose_optimization(p)
    poses = binding.get_poses()
    return {
        "pose7": binding.get_pose_params().copy(),
        "position": np.asarray(poses["position"]).copy(),
        "orientation": np.asarray(poses["orientation"]).copy(),
        "vfov": np.asarray(poses["vfov"]).copy(),
        "hfov": np.asarray(poses["hfov"]).copy(),
        "depth_params": binding.get_xform_params().copy(),
        "grid_size": np.asarray(list(binding.xform_desc().grid_size), np.int32),
        "summary": binding.summary(),
    }


def solution_path(name):
    return os.path.join(SOLUTIONS_DIR, name + ".npz")


def load_solution(name):
    return dict(np.load(solution_path(name), allow_pickle=False))
