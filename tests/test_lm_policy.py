"""The LM driver's two host-side policies (robust_cvd_amd/csrc/cvd_lm.h: TrustRegion, LevelSchedule) without a GPU: a stand-alone
program (tests/lm_policy_main.cpp, which includes that header alone) is compiled with the host compiler, fed a script of events and
answers with radii (hex floats) and decisions."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle.oracle import Oracle
from robust_cvd_amd import synth
from robust_cvd_amd.ctypes_types import OptParams, XformDesc

HERE = os.path.dirname(os.path.abspath(__file__))
KEEP, IN_LINE, SIDE = 0, 1, 2


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = tmp_path_factory.mktemp("lm_policy") / "lm_policy"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-o", str(exe), os.path.join(HERE, "lm_policy_main.cpp")], check=True,
                   capture_output=True, timeout=120)

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True, timeout=30).stdout
        return [ln.split() for ln in out.splitlines()]
    return run


def radii(policy, lines):
    """Script of trust-region events -> [(radius, below_min, gave_up)], one per event."""
    out, res, gave_up = policy(lines), [], False
    for tok in out:
        if tok[0] == "G":
            gave_up = tok[1] == "1"
        elif tok[0] == "R":
            res.append((float.fromhex(tok[1]), tok[2] == "1", gave_up))
            gave_up = False
    assert len(res) == len(lines)
    return res


# ---- (a) trust region, known answers (every value below is exact in binary floating point) ------------------------------
def test_rejections_shrink_by_a_doubling_factor(policy):
    r = radii(policy, ["tr", "reject", "reject", "reject"])
    assert [x[0] for x in r] == [1e4, 5e3, 1.25e3, 156.25]


def test_accepted_steps(policy):
    r = [x[0] for x in radii(policy, ["tr", "accept 0.5", "accept 0.75", "accept 1"])]
    assert r[1] == 1e4                      # 1 - (2 q - 1)^3 = 1
    assert r[2] == 1e4 / 0.875              # 1 - 0.5^3
    assert r[3] == r[2] / (1.0 / 3.0)       # the floor of the divisor


@pytest.mark.parametrize("q", ["0.5", "0.75", "1"])
def test_after_an_accept_the_next_rejection_halves_again(policy, q):
    r = [x[0] for x in radii(policy, ["tr", "reject", "reject", f"accept {q}", "reject", "reject"])]
    assert r[4] == r[3] / 2 and r[5] == r[3] / 8


def test_radius_is_capped(policy):
    r = [x[0] for x in radii(policy, ["tr"] + ["accept 1"] * 40)]
    assert r[-1] == 1e16 and r[-2] == 1e16 and max(r) == 1e16
    assert all(b >= a for a, b in zip(r, r[1:]))


def test_five_invalid_steps_in_a_row_give_up(policy):
    r = radii(policy, ["tr"] + ["invalid"] * 5)
    assert [x[2] for x in r] == [False, False, False, False, False, True]
    assert [x[0] for x in r[:5]] == [1e4, 5e3, 1.25e3, 156.25, 156.25 / 16]   # (an invalid step shrinks like a rejected one)
    assert r[5][0] == r[4][0]                                                # ... the fifth leaves the radius alone
    r = radii(policy, ["tr"] + ["invalid"] * 4 + ["valid"] + ["invalid"] * 4)
    assert not any(x[2] for x in r)
    r = radii(policy, ["tr"] + ["invalid"] * 4 + ["valid"] + ["invalid"] * 5)
    assert [x[2] for x in r] == [False] * 10 + [True]


def test_radius_falls_below_the_minimum(policy):
    r = radii(policy, ["tr"] + ["reject"] * 40)
    below = [x[1] for x in r]
    first = below.index(True)
    assert all(below[first:]) and not any(below[:first])
    assert r[first][0] < 1e-32 <= r[first - 1][0]


def test_stop_tests(policy):
    out = policy(["ptol 1e-8 1.0", "ptol 1.1e-8 1.0", "ftol 2.0 1.999999", "ftol 2.0 1.99999", "ftol 2.0 2.000001", "ftol 2.0 2.00001"])
    assert [t[1] for t in out] == ["1", "0", "1", "0", "1", "0"]


# ---- (b) the oracle's LM run replayed, bit for bit ---------------------------------------------------------------------
def test_radius_replays_the_oracle(policy):
    """Every record of the oracle's normalize_depth run goes through TrustRegion as the driver would feed it: a successful record is
    an accepted step with the record's relative decrease; an unsuccessful one is a rejected step -- unless the driver's parameter /
    function tolerance test says that the solve stopped at it, which leaves the radius alone (the last record here: |step| = 7e-10).  The
    radius must equal the record's exactly: the formulas are the same, `pow` included."""
    v = synth.make_video(8, 64, 40, seed=1)
    o = Oracle()
    synth.load_into(o, v)
    o.reset_depth_xforms(XformDesc.global_depth())
    o.reset_spatial_xforms(XformDesc.spatial())
    o.normalize_depth(OptParams.defaults())
    recs = o.records()
    assert len(recs) == 19 and recs[0]["iteration"] == 0
    assert "".join(str(int(r["step_is_successful"])) for r in recs) == "1000000111111111110"
    # Which unsuccessful records are a solve's stop: asked of the driver's own two tests.  (cost at x, cost of the candidate) come from
    # the record; |x| is that of the final scales -- a stop leaves x where it was, and only a solve's last record can be one.
    x_norm = float(np.linalg.norm(o.get_xform_params()))
    last = recs[-1]
    assert o.summary()["termination"] == 0 and not last["step_is_successful"]
    answers = policy([f"ptol {float(last['step_norm']).hex()} {x_norm.hex()}",
                      f"ftol {float(last['cost']).hex()} {float(last['cost'] - last['cost_change']).hex()}"])
    stopped = {len(recs) - 1} if "1" in (answers[0][1], answers[1][1]) else set()
    assert o.get_xform_params().size == 8 and stopped
    script = []
    for i, r in enumerate(recs):
        if r["iteration"] == 0:
            script.append("tr")
        elif r["step_is_successful"]:
            script.append(f"accept {float(r['relative_decrease']).hex()}")
        else:
            script.append("valid" if i in stopped else "reject")   # (the step that stops a solve is valid and moves nothing)
    for r, g in zip(recs, radii(policy, script)):
        assert g[0] == r["trust_region_radius"], (r["iteration"], g[0].hex(), float(r["trust_region_radius"]).hex())
    # both branches were exercised: six rejections in a row from 1e4, then accepted steps
    assert [r["trust_region_radius"] for r in recs[1:4]] == [5e3, 1.25e3, 156.25]
    assert sum(1 for s in script if s.startswith("accept")) == 11


# ---- (c) the level schedule, known answers transcribed from the LM loop ---------------------------------------------------
def sched(coarse_level=1, temporal_level=0, threshold=16, coarse_on=True, temporal_on=False, dense=False, dist=False, stream3=True,
          small_block=True):
    return "sched " + " ".join(str(int(x)) for x in (coarse_level, temporal_level, threshold, coarse_on, temporal_on, dense, dist,
                                                      stream3, small_block))


def walk(policy, lines):
    """-> one dict per script line that answers: decisions as {"coarse", "aside", "temporal"}, state as {"built", "pending", "fresh",
    "base", "excess"} (a `decide` gives both, merged)."""
    res = []
    for tok in policy(lines):
        if tok[0] == "D":
            res.append({"coarse": int(tok[1]), "aside": tok[2] == "1", "temporal": tok[3] == "1"})
        elif tok[0] == "S":
            st = dict(zip(("built", "pending", "fresh", "base", "excess"), (int(t) for t in tok[1:])))
            if res and "coarse" in res[-1] and "built" not in res[-1]:
                res[-1].update(st)
            else:
                res.append(st)
        elif tok[0] == "T":
            res.append({"threshold": int(tok[1])})
    return res


def test_sparse_factor_excess_rule(policy):
    head = [sched(), "decide", "pcg 30", "decide", "pcg 36", "decide", "pcg 41"]
    w = walk(policy, head)
    assert (w[0]["coarse"], w[0]["aside"], w[0]["fresh"]) == (IN_LINE, True, 1)   # iteration 1: in line, block inverses aside
    assert w[1]["base"] == 30
    assert w[2]["coarse"] == KEEP and not w[2]["aside"] and w[3]["excess"] == 6
    assert w[4]["coarse"] == KEEP and w[5]["excess"] == 17
    # iteration 4, slowly changing regime: on the side stream, this iteration's PCG still runs on the old factor
    w = walk(policy, head + ["rel 0x1.0624dd2f1a9fbp-10", "decide", "pcg 41", "decide", "installed", "decide", "pcg 50", "decide"])[7:]
    assert (w[0]["coarse"], w[0]["aside"], w[0]["temporal"]) == (SIDE, False, False)
    assert (w[0]["pending"], w[0]["fresh"], w[0]["excess"]) == (1, 0, 0)
    assert w[1]["excess"] == 11 and w[1]["base"] == 30           # not fresh: counted against the old base
    assert w[2]["coarse"] == KEEP and w[2]["pending"] == 1       # (while it is pending no decision asks for another rebuild)
    assert (w[3]["pending"], w[3]["fresh"], w[3]["excess"], w[3]["built"]) == (0, 1, 0, 1)   # installed
    assert w[4]["coarse"] == KEEP                                # iteration 5 keeps ...
    assert (w[5]["base"], w[5]["excess"]) == (50, 0)             # ... and its own count is the new base
    assert w[6]["coarse"] == KEEP
    # 0x1.0624dd2f1a9fbp-10 is the double below 1e-3; at 1e-3 itself (or anything above) the rebuild stays in line
    for rel in ("1e-3", "0.5"):
        w = walk(policy, head + [f"rel {rel}", "decide"])[-1]
        assert (w["coarse"], w["aside"], w["fresh"], w["excess"]) == (IN_LINE, True, 1, 0)


def test_no_rebuild_is_asked_for_while_one_is_pending(policy):
    w = walk(policy, [sched(threshold=0), "decide", "pcg 30", "rel 1e-6", "decide", "decide", "pcg 90", "decide"])
    assert [x["coarse"] for x in w if "coarse" in x] == [IN_LINE, SIDE, KEEP, KEEP]


def test_coarse_level_2_rebuilds_in_line_every_iteration(policy):
    w = walk(policy, [sched(coarse_level=2), "rel 1e-6", "decide", "pcg 30", "decide", "pcg 30", "decide"])
    assert [(x["coarse"], x["aside"]) for x in w if "coarse" in x] == [(IN_LINE, True)] * 3


def test_dense_form_is_never_on_the_side_stream(policy):
    w = walk(policy, [sched(dense=True, threshold=32), "rel 1e-6", "decide", "pcg 30", "decide", "pcg 61", "decide", "pcg 62", "decide"])
    assert [x["coarse"] for x in w if "coarse" in x] == [IN_LINE, KEEP, KEEP, IN_LINE]   # (excess 31, then 63)


def test_dense_threshold(policy):
    w = walk(policy, ["thr 0 0 3.0 0.1", "thr 24 0 3.0 0.1", "thr -1 0 3.0 0.1", "thr -1 0 0.1 1.0", "thr -1 0 100.0 0.1", "thr -1 1 3.0 0.1",
                      "thr -1 0 0.0 0.1", "thr -1 0 3.0 0.0", "thr -1 0 1.4 0.1", "thr -1 0 1.3 0.1"])
    # default 32; the option; 1.5 x 30 = 45 -> 48 (steps of 8); clamped to [8, 256]; sharded 32; nothing measured yet 32; 21 -> 24; 19.5 -> 16
    assert [x["threshold"] for x in w] == [32, 24, 48, 8, 256, 32, 32, 32, 24, 16]


def test_sharded_run(policy):
    w = walk(policy, [sched(dist=True, threshold=0), "rel 1e-6", "decide", "pcg 30", "decide", "pcg 40", "decide"])
    assert [(x["coarse"], x["aside"]) for x in w if "coarse" in x] == [(IN_LINE, False)] * 3


@pytest.mark.parametrize("stream3, small_block", [(False, True), (True, False), (False, False)])
def test_block_inverses_aside_need_the_third_stream_and_a_small_block(policy, stream3, small_block):
    w = walk(policy, [sched(stream3=stream3, small_block=small_block), "decide"])
    assert (w[0]["coarse"], w[0]["aside"]) == (IN_LINE, False)


@pytest.mark.parametrize("temporal_level, expect", [(1, [True, False, False, True]), (2, [True, True, True, True])])
def test_depth_grid_level_without_a_pose_graph_level(policy, temporal_level, expect):
    w = walk(policy, [sched(coarse_level=0, coarse_on=False, temporal_on=True, temporal_level=temporal_level), "rel 1e-6",
                      "decide", "pcg 30", "decide", "pcg 36", "decide", "pcg 41", "decide"])
    d = [x for x in w if "coarse" in x]
    assert [(x["coarse"], x["aside"]) for x in d] == [(KEEP, False)] * 4
    assert [x["temporal"] for x in d] == expect
    assert [x["fresh"] for x in d] == [int(e) for e in expect]


def test_no_levels_at_all(policy):
    w = walk(policy, [sched(coarse_level=0, coarse_on=False), "decide", "pcg 30", "decide"])
    assert [(x["coarse"], x["aside"], x["temporal"], x["built"]) for x in w if "coarse" in x] == [(KEEP, False, False, 0)] * 2


def test_temporal_level_2_beside_a_kept_pose_graph_level(policy):
    w = walk(policy, [sched(temporal_on=True, temporal_level=2), "decide", "pcg 30", "decide", "pcg 30", "decide"])
    d = [x for x in w if "coarse" in x]
    assert [(x["coarse"], x["temporal"]) for x in d] == [(IN_LINE, False), (KEEP, True), (KEEP, True)]
    assert [x["fresh"] for x in d] == [1, 0, 0]   # (the kept factor's base count stands)
    w = walk(policy, [sched(temporal_on=True, temporal_level=1), "decide", "pcg 30", "decide"])
    assert [(x["coarse"], x["temporal"]) for x in w if "coarse" in x] == [(IN_LINE, False), (KEEP, False)]
