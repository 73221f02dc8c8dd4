"""numpy float64 restatement of the two spatial losses (robust_cvd_amd/csrc/cvd_spatial.h): the values and the
analytic gradient with respect to the depth table.  Written from the formulas of the reference's
loss/disparity_smooth_loss.py:15-56 and loss/contrast_loss.py:13-79; held against the recorded outputs of the reference itself
by tests/test_spatial_reference.py.
"""
import contextlib
import io
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "spatial_golden.npz")
KINK_DISTANCE = 1e-5        # every |d_a - d_b| and |D_a - D_b| across an edge is at least this
THRESHOLD_DISTANCE = 1e-4   # every original ratio is at least this far from a threshold
MASK_SHARE = (0.10, 0.60)   # share of the edges whose contrast mask is set (every case but `tiny`)


def _edges(a):
    """(left, right) of the x-edges and (top, bottom) of the y-edges of a [..., H, W] table"""
    return (a[..., :, :-1], a[..., :, 1:]), (a[..., :-1, :], a[..., 1:, :])


def _ratio(a, b):
    return np.maximum(a, b) / (np.minimum(a, b) + 1e-10)


def spatial(depth, depth_orig=None, image=None, *, frames_per_sample, lambda_disparity_smooth=0.0, sigma_color_grad=1.0,
            lambda_contrast_loss=0.0, contrast_thresh=1.05, grad=False):
    """(total, smooth [B], contrast) [, d total / d depth [F, H, W]] in float64"""
    D = np.asarray(depth, np.float64)
    H, W = D.shape[-2:]
    D = D.reshape(-1, H, W)
    F, N = D.shape[0], int(frames_per_sample)
    B = F // N
    g = np.zeros_like(D)
    smooth = np.zeros(B)
    contrast = 0.0
    if lambda_disparity_smooth > 0:
        I = np.asarray(image, np.float64).reshape(F, 3, H, W)
        d = 1.0 / D
        for axis, ((da, db), (Ia, Ib)) in enumerate(zip(_edges(d), _edges(I))):
            w = np.exp(-np.mean(np.abs(Ia - Ib), 1) / sigma_color_grad)
            s = w * np.abs(da - db)
            count = N * s.shape[1] * s.shape[2]
            smooth += lambda_disparity_smooth * s.reshape(B, -1).sum(1) / count
            k = lambda_disparity_smooth / (count * B) * w * np.sign(da - db)       # d total / d d_a = -d total / d d_b
            if axis == 0:
                g[:, :, :-1] += k * -(d[:, :, :-1] ** 2)
                g[:, :, 1:] -= k * -(d[:, :, 1:] ** 2)
            else:
                g[:, :-1, :] += k * -(d[:, :-1, :] ** 2)
                g[:, 1:, :] -= k * -(d[:, 1:, :] ** 2)
    if lambda_contrast_loss > 0:
        Do = np.asarray(depth_orig, np.float64).reshape(F, H, W)
        csum = 0.0
        for axis, ((Da, Db), (Oa, Ob)) in enumerate(zip(_edges(D), _edges(Do))):
            mask = _ratio(Oa, Ob) > contrast_thresh
            den = np.minimum(Da, Db) + 1e-10
            hi = np.maximum(Da, Db)
            t = contrast_thresh - hi / den
            csum += np.sum(np.where(mask, t * t, 0.0))
            k = np.where(mask, lambda_contrast_loss / F * -2.0 * t, 0.0)            # d total / d r
            up, dn = 1.0 / den, -hi / (den * den)                                   # d r / d max, d r / d min
            ga = k * np.where(Da > Db, up, np.where(Da < Db, dn, 0.5 * (up + dn)))
            gb = k * np.where(Db > Da, up, np.where(Db < Da, dn, 0.5 * (up + dn)))
            if axis == 0:
                g[:, :, :-1] += ga
                g[:, :, 1:] += gb
            else:
                g[:, :-1, :] += ga
                g[:, 1:, :] += gb
        contrast = lambda_contrast_loss * csum / F
    total = float(np.mean(smooth) + contrast)
    out = (total, smooth, float(contrast))
    if grad:
        out += (g,)
    return out


def check_conditions(case, thresholds):
    """(smallest |d_a - d_b|, smallest |D_a - D_b|, smallest distance of an original ratio from a threshold, {threshold: share of
    the edges with the mask set}) over all edges of a case"""
    D, Do = case["depth"], case["depth_orig"]
    kd = min(float(np.abs(a - b).min()) for a, b in _edges(1.0 / D))
    kD = min(float(np.abs(a - b).min()) for a, b in _edges(D))
    ratios = np.concatenate([_ratio(a, b).ravel() for a, b in _edges(Do)])
    gap = min(float(np.abs(ratios - tau).min()) for tau in thresholds)
    return kd, kD, gap, {tau: float(np.mean(ratios > tau)) for tau in thresholds}


def _options(**kw):
    import types
    return types.SimpleNamespace(**kw)


def reference_run(case, lambda_disparity_smooth, sigma_color_grad, lambda_contrast_loss, contrast_thresh, dtype="float64"):
    """The REAL reference: DisparitySmoothLoss.forward and ContrastLoss.forward (loss/disparity_smooth_loss.py,
    loss/contrast_loss.py) with torch autograd on the CPU, on a case of tests/spatial_cases.py as (B, N, ...) batches; its prints
    are swallowed.  Needs the reference checkout; returns float64 numpy (total, smooth [B], contrast, d total / d depth
    [F, H, W])."""
    import torch
    from tests.reference_residuals import _reference_modules
    _reference_modules()
    from loss.contrast_loss import ContrastLoss
    from loss.disparity_smooth_loss import DisparitySmoothLoss
    td = {"float64": torch.float64, "float32": torch.float32}[dtype]
    opt = _options(distance_type="l1", distance_scale=1.0, lambda_disparity_smooth=lambda_disparity_smooth,
                   sigma_color_grad=sigma_color_grad, lambda_contrast_loss=lambda_contrast_loss,
                   lambda_contrast_thresh=contrast_thresh)
    B, N, H, W = case["B"], case["N"], case["H"], case["W"]
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=td)
    depths = t(case["depth"]).view(B, N, H, W).requires_grad_(True)
    total = torch.zeros((), dtype=td)
    smooth = np.zeros(B)
    contrast = 0.0
    with contextlib.redirect_stdout(io.StringIO()):
        if lambda_disparity_smooth > 0:
            loss, batch = DisparitySmoothLoss(opt)(t(case["image"]).view(B, N, 3, H, W), depths)
            total = total + loss
            smooth = batch["disparity_smooth"].detach().double().numpy().copy()
        if lambda_contrast_loss > 0:
            loss = ContrastLoss(opt)(t(case["depth_orig"]).view(B, N, H, W), depths)
            total = total + loss
            contrast = float(loss.detach().double())
    total.backward()
    return float(total.detach().double()), smooth, contrast, depths.grad.double().numpy().reshape(B * N, H, W).copy()


def joint_reference_run(case, extra, options):
    """The REAL reference's JointLoss.__call__ (loss/joint_loss.py) in float64 on the CPU, on a case of tests/sceneflow_cases.py
    in its own (B, 6) layout with the `extra` inputs of spatial_cases.joint_inputs.  Returns (total, {name: array} of every
    entry of batch_losses, the contrast term, d total / d depth table [F, H, W], [d total / d parameter]).  The reference sums
    its total in a float32 tensor; the per-term values are float64."""
    import torch
    from tests.reference_residuals import _reference_modules
    _reference_modules()
    from loss.joint_loss import JointLoss
    td = torch.float64
    opt = _options(**options)
    assert opt.recon == "colmap"     # (otherwise both geometric modules scale metadata["warp"] in place: the second sees it twice)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=td)
    B, H, W = case["P"], case["H"], case["W"]
    N = case["F"] // B
    assert N == 6 and np.array_equal(case["pairs"], np.arange(B)[:, None] * N + np.arange(2)[None])
    meta = {"extrinsics": t(case["extrinsics"]).view(B, N, 3, 4), "intrinsics": t(case["intrinsics"]).view(B, N, 4),
            "geometry_consistency": {"flows": tuple(t(f) for f in case["flows"]),
                                     "masks": tuple(t(m).view(B, 1, H, W) for m in case["masks"])},
            "temporal_smoothness": {"flows": tuple(t(f) for f in case["nflows"]),
                                    "masks": tuple(t(m).view(B, 1, H, W) for m in case["nmasks"]),
                                    "valid": t(case["valid"]).view(B, 2, 1)}}
    depths = t(case["depth"]).view(B, N, H, W).requires_grad_(True)
    p_init = [t(p) for p in extra["parameters_init"]]
    params = [t(p).requires_grad_(True) for p in extra["parameters"]]
    criterion = JointLoss(opt, p_init)
    with contextlib.redirect_stdout(io.StringIO()):
        loss, batch, _scene_flow = criterion(t(extra["image"]).view(B, N, 3, H, W), t(extra["depth_orig"]).view(B, N, H, W), depths,
                                             meta, params)
        contrast = criterion.contrast_loss(t(extra["depth_orig"]).view(B, N, H, W), depths.detach())
    assert loss.shape == (1,)
    loss.sum().backward()
    batch = {k: v.detach().double().numpy().copy() for k, v in batch.items()}
    return (float(loss.detach().double()[0]), batch, float(contrast), depths.grad.double().numpy().reshape(B * N, H, W).copy(),
            [p.grad.double().numpy().copy() for p in params])
