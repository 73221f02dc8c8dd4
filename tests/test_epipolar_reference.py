"""Known answers for the numpy restatement of the epipolar RANSAC (tests/epipolar_reference.py), which defines
setStaticFlagFromRansac for the GPU parity tests (no GPU needed)."""
import numpy as np
import pytest

from robust_cvd_amd import synth
from tests import epipolar_reference as er
from tests.epipolar_cases import analytic_F, intrinsics, project


def test_splitmix64_and_pinned_draws():
    # the standard SplitMix64 sequence from state 0: mix(golden), mix(2 golden)
    assert er.splitmix64(0) == 0xE220A8397B1DCDAF
    assert er.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert er.draw_sample(0, 0, 0, 600) == [535, 65, 310, 453, 178, 218, 392, 87]
    assert er.draw_sample(0, 3, 5, 50) == [44, 31, 24, 3, 23, 11, 48, 10]
    assert er.draw_sample(7, 1, 2, 8) == [7, 3, 1, 5, 2, 4, 0, 6]
    assert er.draw_sample(0, 0, 0, 7) is None   # 7 constraints never give 8 distinct indices


def two_views(n=300, seed=0, W=384, H=224):
    rng = np.random.default_rng(seed)
    fy = 0.3461538376301239 / (W / H)
    fx = fy * W / H
    K = intrinsics(W, H, fx, fy)
    Ra, ta = synth.rodrigues(np.array([0.01, -0.02, 0.005])), np.array([0.1, 0.0, 0.2])
    Rb, tb = synth.rodrigues(np.array([0.03, 0.04, -0.01])), np.array([0.5, 0.1, -0.2])
    D = rng.uniform(2.0, 6.0, n)
    c = np.stack([rng.uniform(-0.9, 0.9, n) * fx, rng.uniform(-0.9, 0.9, n) * fy, -np.ones(n)], 1)
    X = ta + (D[:, None] * c) @ Ra.T
    return project(X, Ra, ta, K), project(X, Rb, tb, K), analytic_F(Ra, ta, Rb, tb, K)


def test_noise_free_views_recover_the_analytic_F():
    xa, xb, F = two_views()
    r = er.pair_ransac(xa, xb, 1.0, iterations=32, seed=3)
    assert r["best"][1] == xa.shape[0] and r["flags"].all()
    assert np.abs(er.unit_sign(r["F_best"]) - er.unit_sign(F)).max() < 1e-8
    da, db = er.distances(r["F_best"], xa, xb)
    assert max(da.max(), db.max()) < 1e-9
    valid = r["counts"] >= 0
    assert valid.sum() >= 30 and (r["counts"][valid] == xa.shape[0]).all()


def test_closed_form_rank2_equals_the_svd():
    rng = np.random.default_rng(1)
    for _ in range(200):
        F = rng.normal(size=(3, 3))
        a, b = er.rank2_closed_form(F), er.rank2(F)
        assert np.abs(a - b).max() < 1e-10 * np.abs(F).max()
        assert np.linalg.svd(a, compute_uv=False)[2] < 1e-12 * np.abs(F).max()


def test_perpendicular_move_has_that_distance():
    xa, xb, F = two_views(n=20)
    l = np.concatenate([xa, np.ones((20, 1))], 1) @ F.T
    nrm = l[:, :2] / np.linalg.norm(l[:, :2], axis=1, keepdims=True)
    for d in (0.5, 3.0, 7.25):
        da, db = er.distances(F, xa, xb + d * nrm)
        np.testing.assert_allclose(db, d, rtol=0, atol=1e-9)


def test_moved_points_are_flagged_and_degenerate_pairs_stay_static():
    xa, xb, F = two_views(n=200, seed=2)
    rng = np.random.default_rng(5)
    l = np.concatenate([xa, np.ones((200, 1))], 1) @ F.T
    nrm = l[:, :2] / np.linalg.norm(l[:, :2], axis=1, keepdims=True)
    mv = rng.uniform(size=200) < 0.25
    xb2 = xb + rng.normal(0, 0.25, xb.shape) + (mv * rng.uniform(4, 8, 200) * rng.choice([-1, 1], 200))[:, None] * nrm
    r = er.pair_ransac(xa, xb2, 2.0, iterations=128)
    assert (r["flags"][mv] == 0).all() and r["flags"][~mv].all()
    for a, b in ((xa[:7], xb[:7]), (np.tile(xa[:1], (20, 1)), xb[:20])):
        r = er.pair_ransac(a, b, 2.0, iterations=8)
        assert r["best"] == (-1, -1) and r["flags"].all() and (r["counts"] == -1).all()


def test_non_finite_locations_are_rejected():
    loc = np.zeros((10, 4), np.float32)
    loc[3, 2] = np.nan
    with pytest.raises(ValueError):
        er.epipolar_static_flags([0, 10], loc, 96, 2.0)
