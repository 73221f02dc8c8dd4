"""GPU parity (-m gpu) of the segment walk of the frame-major assembly kernel (k_assemble_fast, SPEC 1 / 2, several waves per
workgroup; robust_cvd_amd/csrc/cvd_assembly.h asmWalkSegments, cvd_asm_segments.h).

A wave of a part walks one contiguous run of the part's units, cut into segments (maximal runs of constraints of one (pair, side)
entry); what a segment needs -- its record, the other frame's staged parameters, the first table record -- is requested while the
segment before it is walked.  What that makes fragile is checked here on one problem of 8 frames (96 x 56, a 4 x 3 grid, some frames
rotated by 0.5 - 0.9 rad as in tests/test_gpu_assembly_shapes.py), with the checks and the bar of that file: cost, gradient and the
full frame blocks against the CPU oracle at 1e-9 relative, per frame, the rotation rows on their own, and everything -- the
per-frame costs included -- against the generic kernels.

The product rule gives a part of a few-frame problem at most one unit per wave, so no wave would ever walk two segments: the test
caps the units per part itself (cvd_debug_options::asm_force_part_units = 40, five units per wave in a full part), as the rule does
for the 300-frame workload.  With the per-direction counts below the work list then has (asserted from tests/assembly_segments_model.py,
whose segment count must be the launch's):
  * a wave's run crossing from one entry to the next where the other frame changes, where the other frame stays and the side
    flips ((0, 1) then (1, 0) seen from frame 1), and segments that start in the middle of an entry;
  * segments of 1, 63, 64, 65, 128, 129, 257 and 640 constraints (among others);
  * frame 0 split into two parts; parts with fewer units than waves, so waves without a segment;
  * a frame without constraints (7) and a pair with only its backward direction (5 -> 2).
Every variant runs with 2, 1 and 0 staging rows per wave forced (asm_force_stage_depth), and the launch read-out must report that
depth.  Two sizing cases run the product's own choice at the real block sizes, where alone an LDS overrun would show: B = 177
(17 x 10 grid: two rows fit) and B = 199 (16 x 12: none does).
"""
import numpy as np
import pytest

from oracle.oracle import Oracle
from robust_cvd_amd import synth
from robust_cvd_amd.ctypes_types import OptParams, XformDesc
from tests.assembly_segments_model import properties
from tests.helpers import rel

pytestmark = pytest.mark.gpu

TOL = 1e-9
FRAMES = 8
CAP_UNITS = 40
# directed pair -> constraints kept (found by a search over tests/assembly_segments_model.py for the properties listed above)
COUNTS = {(0, 1): 641, (0, 2): 850, (0, 3): 65, (0, 4): 641, (0, 5): 641, (0, 6): 63, (1, 0): 800, (1, 2): 800, (2, 0): 641,
          (2, 1): 768, (3, 0): 512, (3, 4): 257, (4, 0): 64, (4, 3): 257, (5, 0): 129, (5, 2): 800, (6, 0): 63}
LENGTHS = {1, 63, 64, 65, 128, 129, 257, 640}

VARIANTS = [("cauchy_grid", "grid", 0, 1, 4), ("huber_grid", "grid", 1, 2, 4), ("cauchy_bicubic", "cubic", 0, 1, 16)]
CASES = [(v, d) for v in VARIANTS for d in (2, 1, 0)]


@pytest.fixture(scope="module")
def Solver():
    from robust_cvd_amd import api
    return api.Solver


def _thin(v, counts, seed):
    """Keep counts[(a, b)] constraints of every pair, spread over the image."""
    rng = np.random.default_rng(seed)
    loc, off = [], [0]
    for k, (a, b) in enumerate(map(tuple, v.pairs)):
        have = int(v.offsets[k + 1] - v.offsets[k])
        want = counts[(int(a), int(b))]
        assert have >= want, (a, b, have)
        keep = np.sort(rng.choice(have, want, replace=False)) + int(v.offsets[k])
        loc.append(v.loc[keep])
        off.append(off[-1] + want)
    v.loc = np.concatenate(loc, axis=0)
    v.offsets = np.asarray(off, dtype=np.int64)
    v.is_static = np.ones(v.loc.shape[0], dtype=np.uint8)
    return v


def _poses(frames, rotated, seed):
    rng = np.random.default_rng(seed)
    pose = np.zeros((frames, 7))
    pose[:, :3] = rng.normal(0, 0.05, (frames, 3))
    pose[:, 3:6] = rng.normal(0, 0.05, (frames, 3))
    for f, angle in rotated:
        axis = rng.normal(size=3)
        pose[f, 3:6] = angle * axis / np.linalg.norm(axis)
    pose[:, 6] = 0.2 + rng.uniform(0, 0.02, frames)
    return pose


@pytest.fixture(scope="module")
def problem():
    """(video, pose parameters, what the model says about its work list): built once, never modified."""
    v = _thin(synth.make_video(FRAMES, 96, 56, seed=53, pairs=sorted(COUNTS), spacing=2.0, rot_sigma_deg=2.0), COUNTS, 29)
    assert not (v.pairs == 7).any() and not any((2, 5) == tuple(p) for p in v.pairs)
    pose = _poses(FRAMES, ((0, 0.6), (2, 0.9), (3, 0.5), (5, 0.75), (7, 0.55)), 29)
    pr = properties([tuple(map(int, p)) for p in v.pairs], np.diff(v.offsets).tolist(), FRAMES, CAP_UNITS)
    return v, pose, pr


def test_the_problem_has_the_shapes_the_walk_can_go_wrong_at(problem):
    pr = problem[2]
    print(pr)
    assert LENGTHS <= pr["lengths"]
    assert pr["other_changes"] > 0 and pr["side_flips"] > 0 and pr["mid_entry_starts"] > 0
    assert pr["parts_per_frame"][0] >= 2 and pr["parts_per_frame"][7] == 1
    assert pr["parts_with_fewer_units_than_waves"] > 0 and pr["idle_waves"] > 0
    assert pr["segments"] > FRAMES


def _evaluate(ctor, v, pose, grid, robust, options=None, generic=False):
    s = ctor()
    if options:
        s.set_options(**options)
    synth.load_into(s, v)
    s.reset_depth_xforms(grid)
    s.reset_spatial_xforms(XformDesc.spatial())
    dx = s.get_xform_params()
    s.set_xform_params(0.15 + np.random.default_rng(31).uniform(0, 0.05, dx.shape))
    s.set_robust_loss(robust)
    if generic:
        s.set_generic_kernels(True)
    p = OptParams.defaults()
    p.num_threads = 2
    return s, s.evaluate(p, 0.1, pose, want_hdiag=True)


@pytest.fixture(scope="module")
def references(Solver, problem):
    """Per variant: the oracle's and the generic kernels' evaluation, computed once and shared by the three depths."""
    cache = {}

    def get(depth_kind, robust):
        key = (depth_kind, robust)
        if key not in cache:
            v, pose, _ = problem
            grid = XformDesc.grid_depth(4, 3, cubic=depth_kind == "cubic")
            _, o = _evaluate(Oracle, v, pose, grid, robust)
            sg, g = _evaluate(lambda: Solver(0), v, pose, grid, robust, generic=True)
            launch = sg.assembly_launch_debug()
            assert launch["kind_name"] == "generic"
            cache[key] = (o, g, launch["cost_frame"])
        return cache[key]
    return get


def _compare(h, launch, o, g, cf_g, frames):
    cf_h = launch["cost_frame"]
    print(f"launch { {k: launch[k] for k in launch if k != 'cost_frame'} }  cost rel {abs(h['cost'] - o['cost']) / abs(o['cost']):.2e}  "
          f"gradient rel {rel(h['gradient'], o['gradient']):.2e}  blocks rel {rel(h['hdiag'], o['hdiag']):.2e}  "
          f"rotation rows rel {rel(h['hdiag'][:, 3:6, :], o['hdiag'][:, 3:6, :]):.2e}  vs generic: gradient "
          f"{rel(h['gradient'], g['gradient']):.2e} blocks {rel(h['hdiag'], g['hdiag']):.2e} "
          f"per-frame cost {np.abs(cf_h - cf_g).max() / np.abs(cf_g).max():.2e}")
    assert h["num_residual_blocks"] == o["num_residual_blocks"]
    assert abs(h["cost"] - o["cost"]) <= TOL * abs(o["cost"])
    assert rel(h["gradient"], o["gradient"]) < TOL
    assert rel(h["hdiag"], o["hdiag"]) < TOL
    for f in range(frames):   # (a small frame's error must not hide behind a large frame's block)
        assert rel(h["hdiag"][f], o["hdiag"][f]) < TOL, f
        assert rel(h["gradient"][f], o["gradient"][f]) < TOL, f
    assert rel(h["hdiag"][:, 3:6, :], o["hdiag"][:, 3:6, :]) < TOL
    assert rel(h["gradient"][:, 3:6], o["gradient"][:, 3:6]) < TOL
    assert abs(h["cost"] - g["cost"]) <= TOL * abs(g["cost"])
    assert rel(h["gradient"], g["gradient"]) < TOL
    assert rel(h["hdiag"], g["hdiag"]) < TOL
    assert cf_h.shape == (frames,)
    assert (np.abs(cf_h - cf_g) <= TOL * np.abs(cf_g)).all(), (cf_h, cf_g)
    assert abs(cf_h.sum() - h["cost"]) <= TOL * abs(h["cost"])


@pytest.mark.parametrize("variant,depth", CASES, ids=[f"{v[0]}-depth{d}" for v, d in CASES])
def test_segment_walk_matches_oracle_and_generic_kernels(Solver, problem, references, variant, depth):
    vid, depth_kind, robust, spec, taps = variant
    v, pose, pr = problem
    o, g, cf_g = references(depth_kind, robust)
    grid = XformDesc.grid_depth(4, 3, cubic=depth_kind == "cubic")
    s, h = _evaluate(lambda: Solver(0), v, pose, grid, robust,
                     options={"asm_force_part_units": CAP_UNITS, "asm_force_stage_depth": 1 + depth})
    launch = s.assembly_launch_debug()
    # the instantiation, the forced depth and the work list under test really ran
    assert launch["kind_name"] == "fast list" and launch["spec"] == spec and launch["kd"] == taps, launch
    assert launch["stage_depth"] == depth, launch
    assert launch["segments"] == pr["segments"] and launch["segments"] > FRAMES, (launch, pr)
    assert launch["workgroups"] == pr["parts"] and launch["split_parts"] == pr["parts_per_frame"][0] >= 2, (launch, pr)
    _compare(h, launch, o, g, cf_g, FRAMES)
    assert np.abs(h["gradient"][7, :6]).max() == 0.0   # the frame without constraints carries its regularisers only


@pytest.mark.parametrize("gx,gy,block,depth", [(17, 10, 177, 2), (16, 12, 199, 0)], ids=["B177_two_rows", "B199_no_row"])
def test_staging_depth_follows_the_lds_at_the_real_block_sizes(Solver, gx, gy, block, depth):
    """The product's own choice of the staging depth, at the block sizes where the packed triangle nearly fills the LDS."""
    frames = 4
    v = synth.make_video(frames, 96, 56, seed=11, spacing=3.0, rot_sigma_deg=2.0)
    pose = _poses(frames, ((1, 0.7), (2, 0.5)), 5)
    grid = XformDesc.grid_depth(gx, gy)
    _, o = _evaluate(Oracle, v, pose, grid, 0)
    sg, g = _evaluate(lambda: Solver(0), v, pose, grid, 0, generic=True)
    s, h = _evaluate(lambda: Solver(0), v, pose, grid, 0, options={"asm_force_part_units": 16})
    launch = s.assembly_launch_debug()
    assert h["gradient"].shape == (frames, block)
    assert launch["kind_name"] == "fast list" and launch["spec"] == 1 and launch["kd"] == 4, launch
    assert launch["stage_depth"] == depth and launch["segments"] > frames, launch
    _compare(h, launch, o, g, sg.assembly_launch_debug()["cost_frame"], frames)
