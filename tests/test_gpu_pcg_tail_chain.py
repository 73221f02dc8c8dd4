"""k_pcg_tail's shortened chain (cvd_pcg.h) against the two launches it replaces (cvd_solver_options::pcg_fused_tail = 0), at the shapes
where the new code can go wrong:

  * the finish half asks for the row range and the in-range flag first and leaves the stores of the direction and the product to the
    caller, behind the arrival: rows per frame off the walk's batch of four per 256 threads (hub frames of a sparse list, end frames
    with very few rows), frames without regulariser rows (out of the frame range), triplet rows in the same walk;
  * the first wave of the last workgroup to arrive sums the p.q shares and releases the grid barrier without a workgroup barrier;
  * the temporal levels' workgroups stage their rows of the inverse in LDS in front of the barrier: several node ranges per hat (the
    last one shorter than 11 rows), a level size NT on both sides of the row product's `c + 64 < NT` tail (NT mod 128 in (0, 64] and
    above 64), fewer waves than rows (the Global level's 256-thread workgroups walk several rows each), and the unstaged path
    (cvd_debug_options::tail_no_row_staging) a launch takes when the staged rows do not fit.

The arithmetic is the two-launch path's up to summation order, so the comparisons and bars are those of
test_gpu_parity.py::test_fused_pcg_tail_matches_the_two_launch_path; nothing new is introduced.  The deterministic build
(lib/libcvd_hip_det.so) must repeat a fused solve with both temporal levels bit for bit: the new summation orders are fixed.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from robust_cvd_amd import synth
from robust_cvd_amd.ctypes_types import OptParams, XformDesc
from tests import margins
from tests.helpers import rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DENSE = {"coarse_update_budget": 0, "coarse_over_budget": 1}   # the dense exact pose-graph level
POSE = {"coarse_update_budget": 0, "coarse_over_budget": 0}    # the temporal pose level in its place
DEPTH = {"temporal_level": 2, "temporal_step": 8}              # + the depth-grid level

# name -> (frames, extra_offsets, solver options, set-up).  NT of the temporal pose level = 8 nodes, nodes = ceil((F - 1) / step) + 1.
CASES = {
    # 25 nodes: three node ranges per mode (11 + 11 + 5 rows: the last range is short), NT = 200, NT mod 128 = 72 > 64
    "three_parts_pose": (48, 6, dict(POSE, coarse_temporal_step=2), {}),
    # ... with the depth-grid level beside it (7 nodes every 8 frames)
    "three_parts_pose_and_depth": (48, 6, dict(POSE, coarse_temporal_step=2, **DEPTH), {}),
    # 7 nodes: NT = 56, NT mod 128 in (0, 64]: the row product ends in its single-entry tail
    "row_tail_low": (24, 6, dict(POSE, coarse_temporal_step=4), {}),
    # Global level only: B = 8, 256-thread workgroups, 4 waves for the 7 rows of a mode
    "fewer_waves_than_rows": (24, 6, dict(POSE, coarse_temporal_step=4), {"global_only": True}),
    # a sparse list: hub frames with many partial rows, end frames with very few
    "rows_off_the_batch": (24, 1, dict(DENSE), {}),
    # frames out of the range have no regulariser rows (and their nodes identity rows)
    "frames_out_of_range": (72, 6, {"coarse_level": 3, "coarse_temporal_step": 4, "temporal_level": 2, "temporal_step": 16},
                            {"frame_range": [f for f in range(4, 61) if f not in (17, 18, 19, 40)], "seed": 21}),
    # triplet groups' rows enter the same walk
    "triplets": (24, 6, dict(POSE, coarse_temporal_step=4, **DEPTH), {"triplets": True}),
    # the comparison is not dominated by the eta = 1e-3 stopping rule
    "tight_pcg": (48, 6, dict(POSE, coarse_temporal_step=2, pcg_relative_tolerance=1e-6, **DEPTH), {}),
}


@pytest.fixture(scope="module")
def Solver():
    from robust_cvd_amd import api
    return api.Solver


_RUNS = {}


def solve(Solver, case, fused, no_staging=False):
    """One solve of the case (shared between the tests that need it, never modified)."""
    key = (case, fused, no_staging)
    if key in _RUNS:
        return _RUNS[key]
    F, extra, opts, setup = CASES[case]
    v = synth.make_video(F, 128, 72, seed=setup.get("seed", 14), extra_offsets=extra)
    s = Solver(0)
    synth.load_into(s, v)
    if setup.get("triplets"):
        s.set_triplet_constraints(*synth.make_triplets(v, spacing=20.0))
    s.set_options(pcg_fused_tail=int(fused), tail_no_row_staging=int(no_staging), **opts)
    s.reset_depth_xforms(XformDesc.global_depth())
    s.reset_spatial_xforms(XformDesc.spatial())
    p = OptParams.defaults()
    p.ctf_long, p.ctf_short = 6, 4
    if setup.get("global_only"):
        p.coarse_to_fine, p.num_steps = 0, 1
    if setup.get("triplets"):
        p.smooth_static_weight, p.smooth_dynamic_weight = 0.5, 0.25
    if "frame_range" in setup:
        p.set_frame_range(setup["frame_range"])
    s.normalize_depth(p)
    s.pose_optimization(p)
    cdbg = s.coarse_debug()
    tdbg = s.temporal_debug()
    out = {"summary": s.summary(), "poses": s.get_poses(), "theta": s.get_xform_params().copy(),
           "pcg": [r["linear_iterations"] for r in s.records()], "path": s.path_info(),
           "pose_level_unknowns": 0 if cdbg is None else cdbg["a_c"].shape[0], "depth_level_unknowns": 0 if tdbg is None else tdbg["NT"]}
    s.close()
    _RUNS[key] = out
    return out


def compare(what, a, b, frames=None):
    """The comparisons and bars of test_fused_pcg_tail_matches_the_two_launch_path.  frames: the frame range of the solve (frames
    outside it are untouched and must be identical; the gauge-aligned pose error is taken over the range, as
    test_temporal_levels_with_frames_out_of_range takes it)."""
    sel = slice(None)
    if frames is not None:
        sel = np.array(frames)
        rest = np.setdiff1d(np.arange(len(a["poses"]["position"])), sel)
        assert np.array_equal(a["poses"]["position"][rest], b["poses"]["position"][rest]) and np.array_equal(a["theta"][rest], b["theta"][rest])
    assert a["summary"]["termination"] == 0 and b["summary"]["termination"] == 0
    margins.same_count(f"LM iterations {what}", a["summary"]["num_iterations"], b["summary"]["num_iterations"])
    margins.close_count(f"PCG iterations {what}", sum(a["pcg"]), sum(b["pcg"]), rel=0.15, slack=3)
    fa, fb = a["summary"]["final_cost"], b["summary"]["final_cost"]
    margins.below(f"final cost {what}", abs(fa - fb) / abs(fb), margins.limit(1e-8, 1e-9))
    perr, rerr = synth.relative_pose_error(a["poses"]["position"][sel], a["poses"]["orientation"][sel], b["poses"]["position"][sel],
                                           b["poses"]["orientation"][sel])
    margins.below(f"position {what}", perr, margins.limit(3e-5, 1e-5))
    margins.below(f"rotation {what}", rerr, 2e-4)
    margins.below(f"depth parameters {what}", rel(a["theta"], b["theta"]), margins.limit(3e-5, 1e-5))


@pytest.mark.parametrize("case", list(CASES))
def test_shortened_tail_matches_the_two_launch_path(Solver, case):
    a, b = solve(Solver, case, True), solve(Solver, case, False)
    print(case, "path", a["path"], "pose level NT", a["pose_level_unknowns"], "depth-grid level NT", a["depth_level_unknowns"],
          "PCG", sum(a["pcg"]), "vs", sum(b["pcg"]))
    assert a["path"]["fused_tail"] and not b["path"]["fused_tail"], (a["path"], b["path"])
    opts = CASES[case][2]
    levels = opts.get("coarse_over_budget", 0) == 0 or opts.get("temporal_level", 1) == 2
    if case != "rows_off_the_batch":
        assert a["path"]["pose_graph_level"] == "temporal pose level", a["path"]
    assert a["path"]["tail_rows_staged"] == (levels and case != "rows_off_the_batch"), a["path"]
    # the level sizes the cases were chosen for (NT of the temporal pose level; TlStep::NT of the depth-grid level is printed above)
    nt = a["pose_level_unknowns"]
    if case.startswith("three_parts") or case == "tight_pcg":
        assert nt == 200 and nt % 128 > 64       # 25 nodes: parts of 11, 11 and 5 rows
    if case in ("row_tail_low", "fewer_waves_than_rows", "triplets"):
        assert nt == 56 and 0 < nt % 128 <= 64   # 7 nodes: more rows than the 4 waves of a 256-thread workgroup
    compare(f"fused vs two-launch [{case}]", a, b, frames=CASES[case][3].get("frame_range"))


@pytest.mark.parametrize("case", ["three_parts_pose_and_depth", "fewer_waves_than_rows"])
def test_unstaged_rows_match_the_staged_ones(Solver, case):
    """cvd_debug_options::tail_no_row_staging: the rows from memory behind the barrier (what a launch does whose staged rows would
    not fit the LDS or the device) -- the same products in the same order."""
    a, b = solve(Solver, case, True, no_staging=True), solve(Solver, case, True)
    assert a["path"]["fused_tail"] and not a["path"]["tail_rows_staged"], a["path"]
    assert b["path"]["fused_tail"] and b["path"]["tail_rows_staged"], b["path"]
    compare(f"unstaged vs staged rows [{case}]", a, b)
    compare(f"unstaged rows vs two-launch [{case}]", a, solve(Solver, case, False))


_DET_SCRIPT = r"""
import hashlib, sys
import torch
torch.cuda.init()
from robust_cvd_amd import api, synth
api.load_library(variant="det")
from robust_cvd_amd.ctypes_types import OptParams, XformDesc
v = synth.make_video(48, 128, 72, seed=14, extra_offsets=6)
for rep in range(2):
    s = api.Solver(0)
    synth.load_into(s, v)
    s.set_options(pcg_fused_tail=1, coarse_update_budget=0, coarse_over_budget=0, coarse_temporal_step=2, temporal_level=2, temporal_step=8)
    s.reset_depth_xforms(XformDesc.global_depth())
    s.reset_spatial_xforms(XformDesc.spatial())
    p = OptParams.defaults()
    p.ctf_long, p.ctf_short = 6, 4
    s.normalize_depth(p)
    s.pose_optimization(p)
    sm, info = s.summary(), s.path_info()
    assert info["fused_tail"] and info["tail_rows_staged"], info
    d = lambda a: hashlib.sha256(a.tobytes()).hexdigest()[:16]
    print("rep", rep, "LM", sm["num_iterations"], "pcg", sm["total_linear_iterations"], "cost", float(sm["final_cost"]).hex(),
          "pose", d(s.get_pose_params()), "theta", d(s.get_xform_params()), flush=True)
    s.close()
"""


def test_deterministic_build_repeats_a_fused_solve_with_both_levels_bit_for_bit():
    """(The existing determinism test runs 100 frames, where the exact sparse level keeps the solve on the two-launch tail.)  The
    variant library must be the first load of the library in its process: hence the subprocess."""
    from robust_cvd_amd import build as b
    b.build_deterministic()
    out = subprocess.run([sys.executable, "-c", _DET_SCRIPT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    reps = [l.split(" ", 2)[2] for l in out.stdout.splitlines() if l.startswith("rep ")]
    assert len(reps) == 2, out.stdout
    assert reps[0] == reps[1], "\n".join(reps)
