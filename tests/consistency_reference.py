"""numpy float64 restatement of the consistency loss of flow pairs (robust_cvd_amd/csrc/cvd_consistency.h): the
forward value, the analytic gradient with respect to the depth table, and the per-sample errors.  Written from the formulas of
the reference's loss/consistency_loss.py:92-182, 219-239, utils/geometry.py and utils/loss.py:62-80; held against the recorded
outputs of the reference itself by tests/test_consistency_reference.py.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "consistency_golden.npz")
EPS32 = float(np.finfo(np.float32).eps)
KINK_DISTANCE = 1e-5   # every weighted sample's errors are at least this far from their sign kinks
TERMS = ("reproj", "disp", "depth ratio")


def rho(e, distance, scale, alpha):
    """(rho(e), d rho / d e) of the reference's distance.create: l1 = |e / scale|, the others the exact branch of the general
    robust loss (loss/general.py lossfun) at alpha = 2 (l2), 1 (smooth_l1), 0 (cauchy) or `alpha` (general)."""
    if distance == "l1":
        return np.abs(e / scale), np.sign(e) / scale
    a = {"l2": 2.0, "smooth_l1": 1.0, "cauchy": 0.0, "general": float(alpha)}[distance]
    q = e / scale
    s = q * q
    if a == 2.0:
        return 0.5 * s, q / scale
    if a == 0.0:
        return np.log1p(np.minimum(0.5 * s, 33e37)), (q / scale) / (1.0 + 0.5 * s)
    beta = max(EPS32, abs(a - 2.0))
    a_safe = (1.0 if a >= 0 else -1.0) * max(EPS32, abs(a))
    base = s / beta + 1.0
    return (beta / a_safe) * (base ** (0.5 * a) - 1.0), (a / a_safe) * base ** (0.5 * a - 1.0) * (q / scale)


def _direction(depth, ext, intr, warp, r, t, flow, lam_ratio):
    """Per-sample quantities of one (pair, direction): errors, their derivatives along D_r(x, y) and along z_w, the bilinear taps."""
    H, W = depth.shape[1:]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    px = xx + (warp[r, 0] if warp is not None else 0.0)
    py = yy + (warp[r, 1] if warp is not None else 0.0)
    fxr, fyr, cxr, cyr = intr[r]
    fxt, fyt, cxt, cyt = intr[t]
    ray = np.stack([(px - cxr) / fxr, -(py - cyr) / fyr, -np.ones_like(px)], 0)           # [3, H, W]
    M = ext[t, :, :3].T @ ext[r, :, :3]
    b = ext[t, :, :3].T @ (ext[r, :, 3] - ext[t, :, 3])
    A = np.einsum("ij,jhw->ihw", M, ray)                                                    # d X_t / d D_r
    Xt = A * depth[r][None] + b[:, None, None]
    X, Y, Z = Xt
    projx = cxt + fxt * X / (-Z)
    projy = cyt - fyt * Y / (-Z)
    mx, my = px + flow[0], py + flow[1]
    dx, dy = projx - mx, projy - my
    e_rep = np.sqrt(dx * dx + dy * dy)
    dprojx = -fxt * (A[0] * Z - X * A[2]) / (Z * Z)
    dprojy = fyt * (A[1] * Z - Y * A[2]) / (Z * Z)
    with np.errstate(invalid="ignore", divide="ignore"):
        de_rep = np.where(e_rep > 0, (dx * dprojx + dy * dprojy) / e_rep, 0.0)
    # the reference's `sample`: grid = 2 uv / (size - 1) - 1 into grid_sample (bilinear, align_corners = False, border)
    u = np.clip(mx * W / (W - 1) - 0.5, 0.0, W - 1.0)
    v = np.clip(my * H / (H - 1) - 0.5, 0.0, H - 1.0)
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    tx, ty = u - x0, v - y0
    taps = []
    for (yi, xi, wt) in ((y0, x0, (1 - ty) * (1 - tx)), (y0, x0 + 1, (1 - ty) * tx), (y0 + 1, x0, ty * (1 - tx)),
                         (y0 + 1, x0 + 1, ty * tx)):
        inside = (xi < W) & (yi < H)
        taps.append((np.minimum(yi, H - 1), np.minimum(xi, W - 1), np.where(inside, wt, 0.0)))
    zw = -sum(depth[t][yi, xi] * wt for yi, xi, wt in taps)
    e_dsp = 1.0 / Z - 1.0 / zw
    p, q = np.abs(zw), np.abs(Z)
    e_rat = lam_ratio * np.log(np.minimum(p, q) / np.maximum(p, q))
    sg = np.sign(q - p)      # +1 where |z_w| < |Z|
    return dict(e_rep=e_rep, e_dsp=e_dsp, e_rat=e_rat, de_rep=de_rep, de_dsp=-A[2] / (Z * Z), de_dsp_zw=1.0 / (zw * zw),
                de_rat=-sg * lam_ratio * A[2] / Z, de_rat_zw=sg * lam_ratio / zw, taps=taps)


def consistency(depth, extrinsics, intrinsics, pairs, flow_ab, flow_ba, weight_ab, weight_ba, warp=None, *, distance="l1",
                scale=1.0, alpha=1.0, lambdas=(1.0, 0.0, 100.0), grad=False, samples=False):
    """(total, {term: [P]}) [, d total / d depth [F, H, W]] [, per-sample errors {name: [P, 2, H, W]}] in float64."""
    depth = np.asarray(depth, np.float64)
    ext, intr = np.asarray(extrinsics, np.float64), np.asarray(intrinsics, np.float64)
    warp = None if warp is None else np.asarray(warp, np.float64)
    flows = (np.asarray(flow_ab, np.float64), np.asarray(flow_ba, np.float64))
    F, H, W = depth.shape
    P = len(pairs)
    weights = (np.asarray(weight_ab, np.float64).reshape(P, H, W), np.asarray(weight_ba, np.float64).reshape(P, H, W))
    lam = [float(v) for v in lambdas]
    # mean focal length of the ref frames of ALL pairs, per direction (torch.mean(focal_length(intrinsics_ref)) over the batch)
    fbar = [np.mean(intr[[pr[k] for pr in pairs], :2]) for k in range(2)]
    terms = np.zeros((P, 3))
    g = np.zeros_like(depth)
    err = {k: np.zeros((P, 2, H, W)) for k in ("e_rep", "e_dsp", "e_rat")}
    for p, (a, b) in enumerate(pairs):
        for k, (r, t) in enumerate(((a, b), (b, a))):
            d = _direction(depth, ext, intr, warp, r, t, flows[k][p], lam[2])
            w = weights[k][p]
            n = max(np.sum(w), 1e-6)
            mult = (lam[0], lam[1] * fbar[k], 1.0 if lam[2] > 0 else 0.0)
            gD = np.zeros((H, W))
            gz = np.zeros((H, W))
            for q, name in enumerate(("e_rep", "e_dsp", "e_rat")):
                err[name][p, k] = d[name]
                if lam[q] <= 0:
                    continue
                r_, dr = rho(d[name], distance, scale, alpha)
                terms[p, q] += 0.5 * mult[q] * np.sum(w * r_) / n
                cf = 0.5 * mult[q] / (n * P)
                gD += cf * w * dr * d["de" + name[1:]]
                if q > 0:
                    gz += cf * w * dr * d["de" + name[1:] + "_zw"]
            if grad:
                g[r] += gD
                for yi, xi, wt in d["taps"]:
                    np.add.at(g[t], (yi, xi), -wt * gz)
    total = float(np.mean(np.sum(terms, 1)))
    out = (total, {name: terms[:, q].copy() for q, name in enumerate(TERMS) if lam[q] > 0})
    if grad:
        out += (g,)
    if samples:
        out += (err,)
    return out


def check_kinks(case, lambdas=(1.0, 1.0, 100.0)):
    """Smallest distance of a weighted sample's errors from their sign kinks: (e_rep, |e_dsp|, |e_rat| / lambda_ratio)."""
    from tests.consistency_cases import case_args
    args = case_args(case)
    _t, _terms, err = consistency(*args, lambdas=lambdas, samples=True)
    P, H, W = case["P"], case["H"], case["W"]
    w = np.stack([case["weight_ab"].reshape(P, H, W), case["weight_ba"].reshape(P, H, W)], 1) != 0
    return (float(err["e_rep"][w].min()), float(np.abs(err["e_dsp"][w]).min()), float(np.abs(err["e_rat"][w]).min() / lambdas[2]))


def reference_run(case, distance, scale, alpha, lambdas, dtype="float64"):
    """The REAL reference: ConsistencyLoss.__call__ (loss/consistency_loss.py) with torch autograd on the CPU, on a case of
    tests/consistency_cases.py laid out as its batches (B = P, N = 2).  Needs the reference checkout; returns float64 numpy
    (total, {term: [P]}, d total / d depth table [F, H, W]).

    * For any distance but l1 the reference builds its alpha / scale tensors in its global f32 dtype and asserts it: the f64 run
      constructs the loss with l1 and sets robust_dist to the reference's loss.general.lossfun with f64 tensors.
    * metadata["warp"] is scaled in place by the reference: every call gets a fresh clone.
    * With lambda_static_reprojection = 0 the reference's loop never forms the reprojected points and matched pixels its other
      two branches read, and raises NameError.  Such a combination runs with the reprojection branch on (lambda 1); the total is
      then the mean over the batch of the sum of the terms the combination keeps, through the same autograd graph."""
    import types

    import torch
    from tests.reference_residuals import _reference_modules
    _geometry, ConsistencyLoss = _reference_modules()
    from loss.general import lossfun
    td = {"float64": torch.float64, "float32": torch.float32}[dtype]
    lam = [float(v) for v in lambdas]
    run_lam = list(lam)
    if lam[0] == 0:
        run_lam[0] = 1.0
    f64 = td == torch.float64
    opt = types.SimpleNamespace(distance_type_static="l1" if f64 else distance, distance_scale=scale, distance_alpha=alpha,
                                lambda_static_reprojection=run_lam[0], lambda_static_disparity=run_lam[1],
                                lambda_static_depth_ratio=run_lam[2], recon="colmap" if case["warp"] is None else "i3d")
    loss = ConsistencyLoss(opt)
    if f64 and distance != "l1":
        a = {"l2": 2.0, "smooth_l1": 1.0, "cauchy": 0.0, "general": float(alpha)}[distance]
        a_t, s_t = torch.tensor(a, dtype=td), torch.tensor(float(scale), dtype=td)
        loss.robust_dist = lambda x: lossfun(x, a_t, s_t)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=td)
    idx = torch.tensor(np.asarray(case["pairs"], np.int64))
    P, H, W = case["P"], case["H"], case["W"]
    table = t(case["depth"]).requires_grad_(True)
    meta = {"extrinsics": t(case["extrinsics"])[idx], "intrinsics": t(case["intrinsics"])[idx],
            "geometry_consistency": {"flows": (t(case["flow_ab"]), t(case["flow_ba"])),
                                     "masks": (t(case["weight_ab"]).view(P, 1, H, W), t(case["weight_ba"]).view(P, 1, H, W))}}
    if case["warp"] is not None:
        meta["warp"] = t(case["warp_norm"])[idx].clone()
    total, batch = loss(table[idx], meta)
    if run_lam != lam:
        total = torch.mean(sum(batch[name] for q, name in enumerate(TERMS) if lam[q] > 0))
    total.backward()
    terms = {name: batch[name].detach().double().numpy().copy() for q, name in enumerate(TERMS) if lam[q] > 0}
    return float(total.detach().double()), terms, table.grad.double().numpy().copy()
