"""The fused PCG tail's shares mode (cvd_pcg.h, cvd_kernels.h): k_pcg_tail ends without summing its shares of r^T z, the next product
(k_matvec_pairs_fast<..., SHARES>) sums them in its prologue and closes the iteration's scalars, k_pcg_close closes the last one.

Against the tail that closes itself (cvd_debug_options::tail_closes_scalars = 1) and against the two launches the tail replaces
(cvd_solver_options::pcg_fused_tail = 0), with the shapes, options and bars of tests/test_gpu_pcg_tail_chain.py -- the arithmetic is
theirs up to the order in which the shares of r^T z are summed -- at the shapes where the new code can go wrong:

  * the sum runs over a zero-padded array of 512 words, eight per lane of one wave: share counts on both sides of 64 and of 128 and
    one that is exactly 64 (the counts are printed and asserted);
  * the shares of the dense exact level's parts, of both temporal levels, of one of them, of none;
  * frames out of the range, a tight PCG tolerance, and a PCG stopped by its iteration cap: the closing kernel then finishes the last
    iteration, and the iteration counts of every LM step must be the closing tail's exactly;
  * out of scope -- the Global level (B = 8) and the Huber robustifier (their products have no shares form), triplets, dense mode,
    lockstep -- the tail closes as
    before, and cvd_path_info says so.  (The Global level of every other case's schedule runs that way too, in the same solve as
    shares-mode levels: the two modes alternate on one handle.)

The deterministic build (lib/libcvd_hip_det.so, one-wave product workgroups) must repeat a shares-mode solve bit for bit: the
summation order is fixed.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from robust_cvd_amd import synth
from robust_cvd_amd.ctypes_types import OptParams, XformDesc
from tests.test_gpu_pcg_tail_chain import CASES as CHAIN_CASES, DENSE, DEPTH, POSE, compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (frames, extra_offsets, solver options, set-up, expected share count or None).  Shares: one per frame, one or two per frame
# of the dense exact level (its workgroups' rows, the frame workgroups' rows), hats x node ranges of the depth-grid level, 8 x node
# ranges of the temporal pose level (node ranges = ceil((nodes - 1) / 10), nodes = ceil((F - 1) / step) + 1).
CASES = {name: CHAIN_CASES[name] + (None,) for name in ("three_parts_pose_and_depth", "rows_off_the_batch", "frames_out_of_range",
                                                         "tight_pcg")}
CASES.update({
    "below_64": CHAIN_CASES["row_tail_low"] + (24 + 8,),                       # 7 nodes: one range per mode
    "between_64_and_128": CHAIN_CASES["three_parts_pose"] + (48 + 8 * 3,),     # 25 nodes: three ranges
    "exactly_64": (48, 6, dict(POSE, coarse_temporal_step=4), {}, 48 + 8 * 2),   # 13 nodes: two ranges
    "above_128": (120, 6, dict(POSE, coarse_temporal_step=4), {}, None),  # 31 nodes: three ranges (+ the depth-grid level, on by itself at this length)
})
# the PCG never converges inside its cap: every solve ends in k_pcg_close
CAPPED = {"iteration_cap": (48, 6, dict(POSE, coarse_temporal_step=2, pcg_max_iterations=3, **DEPTH), {}, None)}
OUT_OF_SCOPE = {
    # the Global level (B = 8, one depth tap per side): its shares instantiation is not built (tests/test_codegen_pcg_shares.py)
    "global_level": CHAIN_CASES["fewer_waves_than_rows"] + (None,),
    # the Huber variant of the product (SPEC = 2): its shares forms miss the register budget and are not built
    "huber": (24, 6, dict(POSE, coarse_temporal_step=4, robust_loss=1), {}, None),
    "triplets": CHAIN_CASES["triplets"] + (None,),
    "lockstep": (24, 6, dict(POSE, coarse_temporal_step=4, pcg_lockstep=1), {}, None),
}


@pytest.fixture(scope="module")
def Solver():
    from robust_cvd_amd import api
    return api.Solver


_RUNS = {}


def solve(Solver, name, mode):
    """One solve of the case (shared between the tests, never modified).  mode: 'shares' (the default path), 'closing'
    (tail_closes_scalars = 1), 'two_launch' (pcg_fused_tail = 0)."""
    key = (name, mode)
    if key in _RUNS:
        return _RUNS[key]
    F, extra, opts, setup, _count = {**CASES, **CAPPED, **OUT_OF_SCOPE}[name]
    v = synth.make_video(F, 128, 72, seed=setup.get("seed", 14), extra_offsets=extra)
    s = Solver(0)
    synth.load_into(s, v)
    if setup.get("triplets"):
        s.set_triplet_constraints(*synth.make_triplets(v, spacing=20.0))
    s.set_options(pcg_fused_tail=int(mode != "two_launch"), tail_closes_scalars=int(mode == "closing"), **opts)
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
    out = {"summary": s.summary(), "poses": s.get_poses(), "theta": s.get_xform_params().copy(),
           "pcg": [r["linear_iterations"] for r in s.records()], "path": s.path_info()}
    s.close()
    _RUNS[key] = out
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_shares_mode_matches_the_closing_tail_and_the_two_launches(Solver, name):
    a, b, c = (solve(Solver, name, mode) for mode in ("shares", "closing", "two_launch"))
    print(name, "shares of r^T z:", a["path"]["rz_shares"], "path", a["path"], "PCG", sum(a["pcg"]), "vs closing", sum(b["pcg"]),
          "vs two launches", sum(c["pcg"]))
    assert a["path"]["fused_tail"] and a["path"]["product_sums_shares"] and 0 < a["path"]["rz_shares"] <= 512, a["path"]
    assert b["path"]["fused_tail"] and not b["path"]["product_sums_shares"] and b["path"]["rz_shares"] == 0, b["path"]
    assert not c["path"]["fused_tail"] and not c["path"]["product_sums_shares"], c["path"]
    count = CASES[name][4]
    if count is not None:
        assert a["path"]["rz_shares"] == count, (a["path"], count)
    frames = CASES[name][3].get("frame_range")
    compare(f"shares vs closing tail [{name}]", a, b, frames=frames)
    compare(f"shares vs two-launch [{name}]", a, c, frames=frames)


def test_the_share_counts_lie_where_the_cases_were_chosen_for(Solver):
    counts = {name: solve(Solver, name, "shares")["path"]["rz_shares"] for name in ("below_64", "exactly_64", "between_64_and_128", "above_128")}
    print(counts)
    assert counts["below_64"] < 64 and counts["exactly_64"] == 64 and 64 < counts["between_64_and_128"] < 128 and 128 < counts["above_128"] <= 512


def test_a_pcg_stopped_by_its_cap_is_closed_by_the_closing_kernel(Solver):
    """pcg_max_iterations = 3: no product follows the third tail of a solve; k_pcg_close sums its shares.  S_ITERS (the records'
    linear iterations) must say 3 for every LM step that ran into the cap and the LM trajectory must be the closing tail's: the
    same three iterations were applied."""
    a, b, c = (solve(Solver, "iteration_cap", mode) for mode in ("shares", "closing", "two_launch"))
    print("PCG iterations per LM step: shares", a["pcg"], "closing tail", b["pcg"], "two launches", c["pcg"])
    assert a["path"]["product_sums_shares"] and not b["path"]["product_sums_shares"]
    assert a["pcg"] and max(a["pcg"]) == 3 and max(b["pcg"]) == 3 and max(c["pcg"]) == 3
    assert a["pcg"] == b["pcg"]
    fa, fb = a["summary"]["final_cost"], b["summary"]["final_cost"]
    assert abs(fa - fb) <= 1e-8 * abs(fb), (fa, fb)


@pytest.mark.parametrize("name", list(OUT_OF_SCOPE))
def test_out_of_scope_solves_keep_the_closing_tail(Solver, name):
    a, c = solve(Solver, name, "shares"), solve(Solver, name, "two_launch")
    assert a["path"]["fused_tail"] and not a["path"]["product_sums_shares"] and a["path"]["rz_shares"] == 0, a["path"]
    compare(f"closing tail vs two-launch [{name}]", a, c)


def test_dense_mode_keeps_the_closing_tail(Solver):
    """Dense mode's products (explicit cross blocks, the pixel walk) read beta from the scalars."""
    v = synth.make_video(8, 96, 56, seed=62)
    flow, mask = synth.make_dense_flows(v)
    out = []
    for closing in (0, 1):
        s = Solver(0)
        s.set_options(tail_closes_scalars=closing)
        s.set_video(v.num_frames, v.width, v.height, v.aspect, v.inv_aspect)
        s.set_depth_all(v.depth)
        s.reset_poses()
        s.set_pair_flows(v.pairs, flow, mask)
        p = OptParams.defaults()
        p.ctf_long, p.ctf_short = 6, 4
        s.reset_depth_xforms(XformDesc.global_depth())
        s.reset_spatial_xforms(XformDesc.spatial())
        s.normalize_depth(p)
        s.pose_optimization(p)
        out.append((s.summary(), s.get_xform_params().copy(), s.path_info()))
        s.close()
    assert not out[0][2]["product_sums_shares"] and not out[1][2]["product_sums_shares"], (out[0][2], out[1][2])
    fa, fb = out[0][0]["final_cost"], out[1][0]["final_cost"]
    assert abs(fa - fb) <= 1e-8 * abs(fb) and np.allclose(out[0][1], out[1][1], rtol=3e-5, atol=1e-9)   # (the option changes nothing here)


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
    sm, info, launch = s.summary(), s.path_info(), s.product_launch_debug()
    assert info["fused_tail"] and info["product_sums_shares"] and launch["threads"] == 64, (info, launch)
    d = lambda a: hashlib.sha256(a.tobytes()).hexdigest()[:16]
    print("rep", rep, "LM", sm["num_iterations"], "pcg", sm["total_linear_iterations"], "cost", float(sm["final_cost"]).hex(),
          "pose", d(s.get_pose_params()), "theta", d(s.get_xform_params()), flush=True)
    s.close()
"""


def test_deterministic_build_repeats_a_shares_mode_solve_bit_for_bit():
    """One-wave product workgroups (k_matvec_pairs_fast<4, 64, 1, false, true>: they close in front of their load phase).  The
    variant library must be the first load of the library in its process: hence the subprocess."""
    from robust_cvd_amd import build as b
    b.build_deterministic()
    out = subprocess.run([sys.executable, "-c", _DET_SCRIPT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    reps = [l.split(" ", 2)[2] for l in out.stdout.splitlines() if l.startswith("rep ")]
    assert len(reps) == 2, out.stdout
    assert reps[0] == reps[1], "\n".join(reps)
