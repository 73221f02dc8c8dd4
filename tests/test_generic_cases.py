"""The cases of tests/generic_cases.py, held to their conditions with the oracle alone (no GPU needed).

tests/test_gpu_generic_kernels.py compares the generic <KD, KS> kernels with the oracle on crossings of depth transform, spatial
transform, loss, robustifier and intrinsics mode that the oracle itself was never pinned on.  What makes it a reference there:
its gradient agrees with central differences of its own cost, at each case's own state and over 60 drawn unknowns with the spatial
ones among them (the routine and the bar of tests/test_oracle_problem.test_autodiff_gradient_matches_central_differences).  The
other conditions keep a case where it is meant to be: the <KD, KS> and the frame block it is tabled for, the number of trips a
256-thread workgroup takes over a pair, a spatial transform that the cost and the gradient actually feel, and, for the one-LM-step
cases, a state the oracle accepts a step from, with that step a tenth of the comparison's bar away from a dense solve at most.
"""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import generic_cases as gc
from tests import product_cases as pc
from tests.test_oracle_problem import test_autodiff_gradient_matches_central_differences as central_differences_at_the_small_video


def _evaluate(cid, state=None, **want):
    c = gc.case(cid)
    o = gc.load(Oracle, cid)
    return o, o.evaluate(gc.params(c), 0.1, gc.put(o, gc.problem(cid)[2] if state is None else state), **want)


_FULL = {}


def _full(cid):
    """The oracle's full evaluation at the case's state: computed once."""
    if cid not in _FULL:
        _FULL[cid] = _evaluate(cid, want_hdiag=True, want_hfull=True)[1]
    return _FULL[cid]


@pytest.mark.parametrize("cid", gc.IDS)
def test_taps_and_frame_block(cid):
    c = gc.case(cid)
    assert gc.tap_counts(c.depth(), c.spatial()) == (c.kd, c.ks)
    o = gc.load(Oracle, cid)
    assert o.block_size() == c.block
    n, vertices = gc.num_depth_params(c)
    assert o.get_xform_params().shape == (c.frames, n * vertices)
    assert o.get_xform_params(True).shape == (c.frames, c.block - 7 - n * vertices)
    if cid == "panels_17x10_bicubic":
        assert c.block == 201     # above the 199 unknowns whose packed triangle fits one row panel of k_assemble


def test_every_off_diagonal_instantiation_is_tabled():
    """The six KS != 0 instantiations the golden vectors do not hold at more than one trip -- (1,16), (4,16), (16,4) at all, and
    (1,4), (4,4), (16,16) beyond 256 constraints per pair -- each have a case above 256 constraints per pair."""
    long = {(c.kd, c.ks) for c in gc.CASES if c.ks and c.spacing is not None and c.spacing < 9}
    assert {(1, 16), (4, 16), (16, 4), (1, 4), (4, 4), (16, 16)} <= long
    assert {(1, 4), (4, 4), (16, 16)} <= {(c.kd, c.ks) for c in gc.CASES if c.spacing is None}   # and per work item


@pytest.mark.parametrize("cid", gc.IDS)
def test_constraints_per_pair_stay_in_the_trip_window(cid):
    c = gc.case(cid)
    v, _, _ = gc.problem(cid)
    n = np.diff(v.offsets)
    if c.spacing is None:
        # the work items a 256-CU device gets: three trips of 256 threads, two, one, and a direction that is empty
        longest = [max(m0, m1) for _, _, m0, m1 in pc.expected_items(v, 256)]
        assert len(longest) >= 3 * 256 and max(longest) == 768
        assert sum(256 < m <= 512 for m in longest) >= 4 and sum(m <= 40 for m in longest) >= 700
        assert any(min(m0, m1) == 0 for _, _, m0, m1 in pc.expected_items(v, 256))
        assert 0.05 < 1.0 - v.is_static.mean() < 0.15
        return
    lo, hi = gc.WINDOWS[c.spacing]
    assert n.min() > lo and n.max() <= hi, (int(n.min()), int(n.max()), lo, hi)
    counts = {tuple(p): int(k) for p, k in zip(v.pairs.tolist(), n)}
    assert any(counts.get((b, a), 0) > 0 for (a, b) in counts)     # a pair with both directions
    dynamic = 1.0 - v.is_static.mean()
    assert 0.05 < dynamic < 0.15, dynamic


@pytest.mark.parametrize("cid", gc.IDS)
def test_oracle_is_finite_and_counts_its_residual_blocks(cid):
    c = gc.case(cid)
    v, trip, _ = gc.problem(cid)
    ev = _full(cid)
    assert np.isfinite(ev["cost"]) and np.isfinite(ev["gradient"]).all() and np.isfinite(ev["hfull"]).all()
    assert np.isfinite(ev["hdiag"]).all()
    static = gc.static_constraints_with_valid_depth(v)
    assert 0 < static < int(v.is_static.sum())                      # some constraints meet a zeroed depth pixel
    expected = static + gc.regulariser_blocks(c, gc.params(c))
    if trip is not None:
        nt = gc.triplets_with_valid_depth(v, trip)
        assert 0 < nt < len(trip[2])
        expected += nt
    assert ev["num_residual_blocks"] == expected
    _, cost_only = _evaluate(cid, want_gradient=False)
    assert cost_only["num_residual_blocks"] == expected
    assert abs(cost_only["cost"] - ev["cost"]) <= 1e-14 * abs(ev["cost"])


@pytest.mark.parametrize("cid", gc.SPATIAL_IDS)
def test_the_spatial_transform_is_live(cid):
    c = gc.case(cid)
    pose, dx, sx = gc.problem(cid)[2]
    ev = _full(cid)
    _, flat = _evaluate(cid, state=(pose, dx, np.zeros_like(sx)), want_gradient=False)
    assert abs(flat["cost"] - ev["cost"]) > 1e-3 * abs(ev["cost"])
    g = ev["gradient"]
    first = c.block - sx.shape[1]
    assert np.abs(g[:, first:]).max() >= 1e-6 * np.abs(g).max()
    assert np.abs(np.diag(ev["hfull"]).reshape(c.frames, c.block)[:, first:]).min() > 0.0   # every spatial unknown is reached


@pytest.mark.parametrize("cid", [c.id for c in gc.CASES if c.smooth is not None])
def test_the_triplets_are_live(cid):
    c = gc.case(cid)
    o = gc.load(Oracle, cid)
    off = o.evaluate(gc.params(c, smooth=False), 0.1, gc.put(o, gc.problem(cid)[2]), want_gradient=False)
    assert abs(off["cost"] - _full(cid)["cost"]) > 1e-3 * abs(_full(cid)["cost"])


@pytest.mark.parametrize("cid", gc.IDS)
def test_oracle_gradient_matches_central_differences(cid):
    """At the case's own video and state, robustifier and triplets included; 60 drawn unknowns, 24 on the 110-frame list (its cost
    takes a tenth of a second)."""
    c = gc.case(cid)
    pose, dx, sx = gc.problem(cid)[2]
    o = gc.load(Oracle, cid)
    p = gc.params(c)
    g = _full(cid)["gradient"]
    F, B, nd = c.frames, c.block, dx.shape[1]

    def cost(P, D, S):
        return o.evaluate(p, 0.1, gc.put(o, (P, D, S)), want_gradient=False)["cost"]

    h = 1e-6
    rng = np.random.default_rng(0)
    cols = rng.choice(F * B, size=min(F * B, 60 if c.spacing is not None else 24), replace=False)
    # (the draw must reach the spatial unknowns: 60 of at most 603 columns, a fifth to two thirds of them spatial)
    assert sum(int(k) % B >= 7 + nd for k in cols) >= (3 if c.ks else 0)
    gfd = np.zeros_like(g)
    for k in cols:
        f, j = divmod(int(k), B)

        def pert(sgn):
            P, D, S = pose.copy(), dx.copy(), sx.copy()
            if j < 7:
                P[f, j] += sgn * h
            elif j < 7 + nd:
                D[f, j - 7] += sgn * h
            else:
                S[f, j - 7 - nd] += sgn * h
            return cost(P, D, S)
        gfd[f, j] = (pert(1) - pert(-1)) / (2 * h)
    sel = np.zeros_like(g, dtype=bool)
    sel.ravel()[cols] = True
    err = np.abs(g - gfd)[sel].max() / np.abs(gfd[sel]).max()
    assert err < 5e-6, err
    # the spatial columns on their own scale: they are orders of magnitude below the pose columns
    spatial = sel.copy()
    spatial[:, :7 + nd] = False
    if spatial.any():
        err_s = np.abs(g - gfd)[spatial].max() / np.abs(gfd[spatial]).max()
        assert err_s < 5e-6, err_s
    H = _full(cid)["hfull"]
    np.testing.assert_allclose(H, H.T, atol=0)
    assert np.linalg.eigvalsh(H).min() > -1e-8 * np.abs(H).max()


@pytest.mark.parametrize("cid", gc.SPATIAL_IDS)
def test_oracle_gradient_at_the_descriptors_of_the_case(cid):
    """tests/test_oracle_problem's own routine (its video, its state) with the case's descriptors, intrinsics mode and loss."""
    c = gc.case(cid)
    central_differences_at_the_small_video(cid, c.depth(), c.spatial(), c.intr, c.loss)


@pytest.mark.parametrize("cid", gc.LM_IDS)
def test_the_oracle_accepts_the_lm_step_and_solves_its_system(cid):
    """The conditions of the one-LM-step comparison: the oracle accepts the step from gc.lm_state, and that step is the solution of
    the damped system of its own J^T J and gradient: ten times its distance from a dense numpy solve stays below the comparison's
    bar of 1e-6 (the condition `oracle_vs_dense_solve` of tests/test_gpu_product_shapes.test_one_lm_step_matches_the_exact_step)."""
    c = gc.case(cid)
    state, advanced = gc.lm_state(cid)
    assert advanced == {"global_bicubic": 8, "grid4x3_bicubic_ratio": 0, "cubic4x4_bilinear_shared_huber": 10}[cid]
    o = gc.load(Oracle, cid)
    ev = o.evaluate(gc.params(c), 0.1, gc.put(o, state), want_hfull=True)
    step, accepted, sm = gc.one_lm_iteration(o, c, state)
    assert sm["num_iterations"] == 1 and accepted, sm
    ref = np.linalg.norm(step)
    assert ref > 0.0
    first = c.block - state[2].shape[1]
    assert np.abs(step[:, first:]).max() > 0.0                      # the spatial unknowns move
    exact = gc.dense_lm_step(ev["hfull"], ev["gradient"]).reshape(c.frames, c.block)
    assert 10.0 * np.linalg.norm(step - exact) / ref < 1e-6, np.linalg.norm(step - exact) / ref
