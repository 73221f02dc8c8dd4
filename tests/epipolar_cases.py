"""Geometry for the epipolar RANSAC tests (tests/test_gpu_epipolar.py, tests/test_epipolar_reference.py): the analytic
fundamental matrix of the synthetic camera model of robust_cvd_amd/synth.py and the projection it implies.

Camera model of robust_cvd_amd/synth.py: q = R^T (X - t) (camera looks along -z), pixel x = (q.x / (z fx) + 1) W / 2,
y = (1 - q.y / (z fy)) H / 2 with z = -q.z (image y down).  So x_h ~ K q with K = [[W / (2 fx), 0, -W / 2],
[0, -H / (2 fy), -H / 2], [0, 0, -1]], and for q_b = R q_a + t (R = R_b^T R_a, t = R_b^T (t_a - t_b)):
F = K^-T [t]x R K^-1 with x_b^T F x_a = 0.
"""
import numpy as np

from robust_cvd_amd import synth


def intrinsics(W, H, fx, fy):
    return np.array([[W / (2 * fx), 0.0, -W / 2.0], [0.0, -H / (2 * fy), -H / 2.0], [0.0, 0.0, -1.0]])


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def analytic_F(Ra, ta, Rb, tb, K):
    R = Rb.T @ Ra
    t = Rb.T @ (ta - tb)
    Ki = np.linalg.inv(K)
    return Ki.T @ skew(t) @ R @ Ki


def project(X, R, t, K):
    q = (X - t) @ R   # R^T (X - t)
    h = q @ K.T
    return h[:, :2] / h[:, 2:3]


def moving_object_video(num_frames=10, width=384, height=224, seed=5, focal_long=2.0, trans_sigma=0.6, gap=(2, 3),
                        region=(0.6, 0.8, 0.25, 0.65), move_px=(6.0, 10.0)):
    """A synth.make_video scene (static flow noise 0.25 px) with a "moving object": every constraint whose source pixel lies
    in the image rectangle `region` (x0, x1, y0, y1 as fractions of W / H) has its target moved U(move_px) px (to one side
    per pair, as a rigid object's motion would) perpendicular to its true epipolar line, computed from the generator's poses.  The pairs are the frame gaps in `gap`.

    The wide field of view (focal_long 2 against the default 0.35) makes every view hold several walls of the box room: at
    the default, a view is mostly the far wall, a plane, on which F is ill-posed and a wrong F can absorb the moved
    constraints.  The baseline (trans_sigma, gap) gives a median static parallax (|x_b - H_inf x_a|, the displacement due
    to translation alone) of >= 10 px, asserted here.  Returns (video with the moved loc, moved [C] bool, parallax [C])."""
    pairs = [(a, b) for a in range(num_frames) for b in range(num_frames) if abs(a - b) in gap]
    v = synth.make_video(num_frames, width, height, seed=seed, pairs=pairs, trans_sigma=trans_sigma, focal_long=focal_long)
    fy = v.true_fy
    fx = fy * float(v.aspect)
    K = intrinsics(width, height, fx, fy)
    Ki = np.linalg.inv(K)
    R = synth.rodrigues(v.true_w)
    t = v.true_t
    rng = np.random.default_rng(seed + 1)
    W, H = width, height
    moved = np.zeros(v.num_constraints, bool)
    parallax = np.zeros(v.num_constraints)
    for p, (a, b) in enumerate(np.asarray(v.pairs).tolist()):
        s, e = int(v.offsets[p]), int(v.offsets[p + 1])
        xa = v.loc[s:e, 0:2].astype(np.float64) * W
        xb = v.loc[s:e, 2:4].astype(np.float64) * W
        ha = np.concatenate([xa, np.ones((e - s, 1))], 1)
        h = ha @ (K @ R[b].T @ R[a] @ Ki).T
        parallax[s:e] = np.linalg.norm(xb - h[:, :2] / h[:, 2:3], axis=1)
        sel = (xa[:, 0] >= region[0] * W) & (xa[:, 0] < region[1] * W) & (xa[:, 1] >= region[2] * H) & \
              (xa[:, 1] < region[3] * H)
        l = ha @ analytic_F(R[a], t[a], R[b], t[b], K).T
        nrm = l[:, :2] / np.linalg.norm(l[:, :2], axis=1, keepdims=True)
        d = rng.uniform(move_px[0], move_px[1], e - s) * rng.choice([-1.0, 1.0])   # the object moves one way per pair
        v.loc[s:e, 2:4] = np.where(sel[:, None], (xb + d[:, None] * nrm) / W, v.loc[s:e, 2:4]).astype(np.float32)
        moved[s:e] = sel
    assert np.median(parallax[~moved]) >= 10.0, np.median(parallax[~moved])
    assert 0.05 < moved.mean() < 0.4, moved.mean()
    return v, moved, parallax


def true_fov(video, focal_long):
    """(vFov, hFov) of the generator's camera, as DvpoParams::focalLong sets them (reference lib/PoseOptimizer.cpp)."""
    A = float(video.aspect)
    return (2.0 * np.arctan(focal_long / A), 2.0 * np.arctan(focal_long)) if A >= 1.0 else \
        (2.0 * np.arctan(focal_long), 2.0 * np.arctan(focal_long * A))


def true_quaternions(video):
    n = np.linalg.norm(video.true_w, axis=1, keepdims=True)
    return np.concatenate([np.sin(n / 2) * video.true_w / np.maximum(n, 1e-30), np.cos(n / 2)], axis=1)
