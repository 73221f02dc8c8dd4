"""GPU tests (-m gpu) of the epipolar RANSAC (robust_cvd_amd/csrc/cvd_epipolar.h, cvd_epipolar_static_flags,
FlowConstraintsCollection::setStaticFlagFromRansac) against its numpy restatement tests/epipolar_reference.py."""
import importlib
import os
import sys

import numpy as np
import pytest

from robust_cvd_amd import synth
from tests import epipolar_reference as er
from tests.epipolar_cases import analytic_F, intrinsics, moving_object_video, project, true_fov, true_quaternions

pytestmark = pytest.mark.gpu

W, H = 384, 224


@pytest.fixture(scope="module")
def solver():
    from robust_cvd_amd import api
    return api.Solver(0)


def scene_pair(n, seed, moved_fraction=0.2, noise=0.25):
    """n correspondences of random-depth points between two views of the synth camera model; a fraction moved 4-8 px
    perpendicular to the true epipolar line.  Returns loc [n, 4] float32 (the collection's convention: pixel / W)."""
    rng = np.random.default_rng(seed)
    fy = 0.3461538376301239 / (W / H)
    fx = fy * W / H
    K = intrinsics(W, H, fx, fy)
    Ra, ta = synth.rodrigues(rng.normal(0, 0.02, 3)), rng.normal(0, 0.1, 3)
    Rb, tb = synth.rodrigues(rng.normal(0, 0.02, 3)), ta + np.array([0.4, 0.05, -0.2]) + rng.normal(0, 0.05, 3)
    D = rng.uniform(2.0, 6.0, n)
    c = np.stack([rng.uniform(-0.95, 0.95, n) * fx, rng.uniform(-0.95, 0.95, n) * fy, -np.ones(n)], 1)
    X = ta + (D[:, None] * c) @ Ra.T
    xa, xb = np.rint(project(X, Ra, ta, K)), project(X, Rb, tb, K) + rng.normal(0, noise, (n, 2))
    F = analytic_F(Ra, ta, Rb, tb, K)
    l = np.concatenate([xa, np.ones((n, 1))], 1) @ F.T
    nrm = l[:, :2] / np.linalg.norm(l[:, :2], axis=1, keepdims=True)
    mv = rng.uniform(size=n) < moved_fraction
    xb = xb + (mv * rng.uniform(4, 8, n) * rng.choice([-1.0, 1.0], n))[:, None] * nrm
    return (np.concatenate([xa, xb], 1) / W).astype(np.float32), mv


def collection(sizes, seed=0):
    locs, moved = zip(*[scene_pair(n, seed + i) for i, n in enumerate(sizes)])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return off, np.concatenate(locs), np.concatenate(moved)


def well_conditioned(na, nb, idx):
    s = np.linalg.svd(er.design_rows(na[idx], nb[idx]), compute_uv=False)
    return s[7] >= 1e-6 * s[0]


def test_per_hypothesis_parity_with_the_restatement(solver):
    sizes = [8, 9, 50, 600, 3000, 20000]
    off, loc, _ = collection(sizes, seed=12)   # (data whose restated distances all lie > 1e-6 px from the threshold)
    K, thr, seed = 256, 2.0, 5
    flags, F, best, counts, hyp = solver.epipolar_debug(off, loc, W, thr, K, seed)
    rf, rF, rbest, res = er.epipolar_static_flags(off, loc, W, thr, K, seed)
    compared = 0
    for p, n in enumerate(sizes):
        r = res[p]
        a, b = int(off[p]), int(off[p + 1])
        xa, xb = er.pixels(loc[a:b], W)
        na, nb = er.apply(r["Ta"], xa), er.apply(r["Tb"], xb)
        for k in range(K):
            idx = er.draw_sample(seed, p, k, n)
            if idx is None or r["counts"][k] < 0 or not well_conditioned(na, nb, idx):
                continue
            assert counts[p, k] >= 0, (p, k)
            assert np.abs(er.unit_sign(hyp[p, k]) - er.unit_sign(r["F"][k])).max() < 1e-8, (p, k)
            da, db = er.distances(r["F"][k], xa, xb)
            assert np.abs(np.maximum(da, db) - thr).min() > 1e-6, (p, k)   # no restated decision is ambiguous
            assert counts[p, k] == r["counts"][k], (p, k)
            compared += 1
        assert tuple(best[p]) == tuple(r["best"]), p
        da, db = er.distances(r["F_best"], xa, xb)
        assert np.abs(np.maximum(da, db) - thr).min() > 1e-6, p
        assert np.abs(er.unit_sign(F[p]) - er.unit_sign(r["F_best"])).max() < 1e-7, p
    assert compared > 0.9 * K * len(sizes)
    np.testing.assert_array_equal(flags, rf)


def test_degenerate_pairs_and_bad_arguments(solver):
    good, _ = scene_pair(40, 1)
    same = np.tile(good[:1], (30, 1))
    line = np.zeros((30, 4), np.float32)   # collinear on both sides
    line[:, 0] = line[:, 2] = np.linspace(0.1, 0.9, 30)
    line[:, 1] = line[:, 3] = 0.3
    loc = np.concatenate([good[:5], same, line, good])
    off = np.array([0, 5, 35, 65, 105], np.int64)
    flags, F, best = solver.epipolar_static_flags(off, loc, W, 2.0, 64)
    assert flags[:35].all() and tuple(best[0]) == (-1, -1) and tuple(best[1]) == (-1, -1)
    assert np.all(F[0] == 0) and np.all(F[1] == 0)
    assert flags[35:65].all() or best[2][0] >= 0   # collinear: every hypothesis is invalid (all static) or a valid F fits
    rf, _, rbest, _ = er.epipolar_static_flags(off, loc, W, 2.0, 64)
    np.testing.assert_array_equal(flags, rf)
    assert (best == rbest).all()
    for kw, word in ((dict(threshold=0.0), "threshold"), (dict(threshold=float("nan")), "threshold"),
                     (dict(iterations=0), "iterations"), (dict(iterations=65537), "iterations")):
        args = dict(threshold=2.0, iterations=64)
        args.update(kw)
        with pytest.raises(RuntimeError, match=word):
            solver.epipolar_static_flags(off, loc, W, args["threshold"], args["iterations"])
    bad = loc.copy()
    bad[40, 3] = np.inf
    with pytest.raises(RuntimeError, match="non-finite"):
        solver.epipolar_static_flags(off, bad, W, 2.0, 64)
    # the handle still works after the rejections
    f2, _, _ = solver.epipolar_static_flags(off, loc, W, 2.0, 64)
    np.testing.assert_array_equal(f2, flags)
    e, _, _ = solver.epipolar_static_flags(np.zeros(1, np.int64), np.zeros((0, 4), np.float32), W, 2.0, 64)
    assert e.shape == (0,)


def test_bitwise_repeat(solver):
    off, loc, _ = collection([600, 1500, 90], seed=21)
    a = solver.epipolar_static_flags(off, loc, W, 2.0, 1024, 9)
    b = solver.epipolar_static_flags(off, loc, W, 2.0, 1024, 9)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_detection_of_moved_constraints(solver):
    """A synth.make_video scene (median static parallax >= 10 px) whose "moving object" constraints are moved 6-10 px
    perpendicular to their true epipolar lines (tests/epipolar_cases.py)."""
    v, moved, _ = moving_object_video()
    flags, F, best = solver.epipolar_static_flags(v.offsets, v.loc, v.width, 2.0)
    st = flags.astype(bool)
    recall = (~st[moved]).mean()
    fpr = (~st[~moved]).mean()
    assert recall >= 0.98 and fpr <= 0.005, (recall, fpr)


def test_too_many_pairs_are_rejected_before_any_work(solver):
    P = 1 << 20
    with pytest.raises(RuntimeError, match="num_pairs"):
        solver.epipolar_static_flags(np.zeros(P + 1, np.int64), np.zeros((0, 4), np.float32), W, 2.0, 16)


@pytest.fixture(scope="module")
def lib():
    from robust_cvd_amd import build as _b
    d = os.path.dirname(_b.build_lib_python())
    if d not in sys.path:
        sys.path.insert(0, d)
    return importlib.import_module("lib_python")


def ransac_pose_optimizer(lib, base_dir, model_type, thresh):
    """PoseOptimizer.__init__ (reference pose_optimization.py:99-175) with opt.dynamic_constraints == "Ransac"."""
    CV_8UC1, CV_32FC3 = 0, 21
    dv = lib.DepthVideo()
    lib.DepthVideoImporter.importVideo(dv, base_dir, False)
    dv.createColorStream("full", "color_full", ".png", CV_32FC3)
    dv.createColorStream("down", "color_down", ".raw", CV_32FC3)
    depth_tag = f"depth_{model_type}"
    dv.createDepthStream(depth_tag, depth_tag, [-1, -1])
    dv.save()
    fcp = lib.FlowConstraintsParams()
    fcp.frameRange.resolve(dv.numFrames(), True)
    fc = lib.FlowConstraintsCollection(dv, fcp)
    fc.setStaticFlagFromRansac(thresh)
    fc.save()
    return dv, fc


def drop_in_solve(lib, video, base, focal_long, ransac):
    """PoseOptimizer.__init__ (Ransac: the restatement above; else tests/drop_in_caller.py's, which leaves every flag static
    without a dynamic_mask stream) and optimize_poses().  The frames start at the generator's field of view."""
    from tests.drop_in_caller import build_pose_optimizer, optimize_poses
    frames = list(range(video.num_frames))
    opt = lib.DepthVideoPoseOptimizer.Params()
    opt.ctfLong, opt.ctfShort = 6, 4
    opt.focalLong = focal_long
    dv, fc = ransac_pose_optimizer(lib, base, "midas2", 2.0) if ransac else build_pose_optimizer(lib, base, "midas2", frames, opt)
    vf, hf = true_fov(video, focal_long)
    ds = dv.depthStream(0)
    for f in frames:
        fr = ds.frame(f)
        it = fr.intrinsics
        it.vFov, it.hFov = vf, hf
        fr.intrinsics = it
    flags = np.concatenate([np.asarray(fc.staticFlags(int(a), int(b)), np.uint8) for a, b in video.pairs])
    optimize_poses(lib, dv, fc, frames, opt)
    pos = np.stack([np.asarray(ds.frame(f).extrinsics.position) for f in frames])
    quat = np.stack([np.asarray(ds.frame(f).extrinsics.orientation.coeffs()) for f in frames])
    depth = np.stack([np.asarray(ds.frame(f).sourceDepth()) for f in frames])
    return flags, pos, quat, depth, dv


def test_drop_in_ransac_improves_the_poses_and_matches_the_oracle(lib, solver, tmp_path):
    """--opt.dynamic_constraints Ransac through the drop-in on the moving-object video: the flags are the C ABI's, the
    poses are closer to the ground truth than with every constraint static, and the end state is the oracle's solve given
    the same flags (set up as in tests/test_gpu_parity.py)."""
    from oracle.oracle import Oracle
    from robust_cvd_amd import dataset_io
    from robust_cvd_amd.ctypes_types import OptParams, XformDesc
    focal = 2.0
    v, moved, _ = moving_object_video(focal_long=focal)
    tq = true_quaternions(v)
    flags_c, _, _ = solver.epipolar_static_flags(v.offsets, v.loc, v.width, 2.0)
    res = {}
    for name, ransac in (("ransac", True), ("static", False)):
        base = dataset_io.write_dataset(str(tmp_path / name), v)
        res[name] = drop_in_solve(lib, v, base, focal, ransac)
    np.testing.assert_array_equal(res["ransac"][0], flags_c)
    assert res["static"][0].all()
    err = {k: synth.relative_pose_error(r[1], r[2], v.true_t, tq) for k, r in res.items()}
    assert err["ransac"][0] < err["static"][0] and err["ransac"][1] < err["static"][1], err
    # the oracle on the same inputs and flags
    frames = list(range(v.num_frames))
    _, pos, quat, depth, dv = res["ransac"]
    vf, hf = true_fov(v, focal)
    o = Oracle()
    o.set_video(v.num_frames, v.width, v.height, dv.aspect(), dv.invAspect())
    o.set_depth_all(depth)
    o.set_pair_constraints(v.pairs, v.offsets, v.loc, flags_c)
    o.set_poses(np.zeros((len(frames), 3)), np.tile([0, 0, 0, 1.0], (len(frames), 1)), [vf] * len(frames), [hf] * len(frames))
    p = OptParams.defaults()
    p.num_threads = 8
    p.ctf_long, p.ctf_short = 6, 4
    p.focal_long = focal
    p.set_frame_range(frames)
    o.reset_depth_xforms(XformDesc.global_depth())
    o.reset_spatial_xforms(XformDesc.spatial())
    o.normalize_depth(p)
    o.pose_optimization(p)
    po = o.get_poses()
    perr, rerr = synth.relative_pose_error(pos, quat, po["position"], po["orientation"])
    assert perr < 1e-3 and rerr < 1e-3, (perr, rerr, err)


def test_drop_in_requires_the_down_stream(lib, tmp_path):
    from robust_cvd_amd import dataset_io
    v = synth.make_video(6, 96, 56, seed=9)
    base = dataset_io.write_dataset(str(tmp_path / "video"), v)
    dv = lib.DepthVideo()
    lib.DepthVideoImporter.importVideo(dv, base, False)
    dv.createDepthStream("depth_midas2", "depth_midas2", [-1, -1])
    fcp = lib.FlowConstraintsParams()
    fcp.frameRange.resolve(dv.numFrames(), True)
    fc = lib.FlowConstraintsCollection(dv, fcp)
    with pytest.raises(RuntimeError, match="'down'"):
        fc.setStaticFlagFromRansac(2.0)
