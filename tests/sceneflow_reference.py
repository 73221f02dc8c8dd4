"""numpy float64 restatement of the scene-flow loss of flow pairs (robust_cvd_amd/csrc/cvd_sceneflow.h): the
forward value, the analytic gradient with respect to the depth table, the six visualisation maps and the per-sample errors.
Written from the formulas of the reference's loss/scene_flow_loss.py:31-356, utils/geometry.py and utils/loss.py:62-80; held
against the recorded outputs of the reference itself by tests/test_sceneflow_reference.py.
"""
import os

import numpy as np

from tests.consistency_reference import rho

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "sceneflow_golden.npz")
KINK_DISTANCE = 1e-5   # every weighted sample's errors are at least this far from their sign kinks
TERMS = ("static", "smooth_reproj", "smooth_disparity", "smooth_depth_ratio")


def _grid(H, W):
    return np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")


def _rays(intr, warp, f, H, W):
    """(pix x, pix y, ray [3, H, W]) of frame f"""
    yy, xx = _grid(H, W)
    px = xx + (warp[f, 0] if warp is not None else 0.0)
    py = yy + (warp[f, 1] if warp is not None else 0.0)
    fx, fy, cx, cy = intr[f]
    return px, py, np.stack([(px - cx) / fx, -(py - cy) / fy, -np.ones_like(px)], 0)


def _sample(depth, intr, warp, f, mx, my):
    """S_f(m): the bilinear sample of frame f's camera-space point map [3, H, W] at pixel positions m, and its taps
    (row, column, weight): the reference's `sample` -- grid = 2 m / (size - 1) - 1 into grid_sample (bilinear, align_corners =
    False, border)."""
    H, W = depth.shape[1:]
    _px, _py, ray = _rays(intr, warp, f, H, W)
    pts = ray * depth[f][None]
    u = np.clip(mx * W / (W - 1) - 0.5, 0.0, W - 1.0)
    v = np.clip(my * H / (H - 1) - 0.5, 0.0, H - 1.0)
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    tx, ty = u - x0, v - y0
    taps = []
    for (yi, xi, wt) in ((y0, x0, (1 - ty) * (1 - tx)), (y0, x0 + 1, (1 - ty) * tx), (y0 + 1, x0, ty * (1 - tx)),
                         (y0 + 1, x0 + 1, ty * tx)):
        inside = (xi < W) & (yi < H)
        taps.append((np.minimum(yi, H - 1), np.minimum(xi, W - 1), np.where(inside, wt, 0.0)))
    S = sum(pts[:, yi, xi] * wt[None] for yi, xi, wt in taps)
    return S, taps, ray


def _scatter(g, f, taps, ray, u):
    """adds weight_tap ray(tap) . u to g[f] for the gradient u [3, H, W] (frame f's camera) of the sampled points"""
    for yi, xi, wt in taps:
        np.add.at(g[f], (yi, xi), wt * np.sum(ray[:, yi, xi] * u, 0))


def scene_flow(depth, extrinsics, intrinsics, pair_frames, flows=None, masks=None, neighbor_frames=None, neighbor_flows=None,
               neighbor_masks=None, valid=None, warp=None, *, distance_static="l1", distance_smooth="l1", scale=1.0, alpha=1.0,
               lambdas=(1.0, 1.0, 0.0, 100.0), grad=False, maps=False, samples=False, weight_is_data=False):
    """(total, {term: [P]}) [, d total / d depth [F, H, W]] [, maps [6, P, 3, H, W]] [, per-sample errors] in float64.
    weight_is_data: the gradient that treats the static weight mask / |D| as a constant (wrong on purpose; the tests show that the
    fixture tells it from the right one)."""
    depth = np.asarray(depth, np.float64)
    ext, intr = np.asarray(extrinsics, np.float64), np.asarray(intrinsics, np.float64)
    warp = None if warp is None else np.asarray(warp, np.float64)
    F, H, W = depth.shape
    pairs = np.asarray(pair_frames).reshape(-1, 2)
    P = len(pairs)
    lam = [float(v) for v in lambdas]
    R, t = ext[:, :, :3], ext[:, :, 3]
    terms = np.zeros((P, 4))
    g = np.zeros_like(depth)
    out_maps = np.zeros((6, P, 3, H, W))
    err = {k: np.zeros((P, 2, H, W)) for k in ("d", "e_rep", "e_dsp", "z_gap")}
    f64 = lambda a: np.asarray(a, np.float64)
    if lam[0] > 0:
        for p, (a, b) in enumerate(pairs):
            for k, (r, tg) in enumerate(((a, b), (b, a))):
                px, py, ray = _rays(intr, warp, r, H, W)
                D = depth[r]
                A = np.einsum("ij,jhw->ihw", R[r], ray)                        # d Xw_r / d D_r
                Xw = A * D[None] + t[r][:, None, None]
                S, taps, ray_t = _sample(depth, intr, warp, tg, px + f64(flows[k][p])[0], py + f64(flows[k][p])[1])
                Y = np.einsum("ij,jhw->ihw", R[tg], S) + t[tg][:, None, None]
                v = Xw - Y
                d = np.sqrt(np.sum(v * v, 0))
                m = f64(masks[k][p]).reshape(H, W)
                w = m / np.abs(D)
                sw, n = np.sum(w), max(np.sum(w), 1e-6)
                r_, dr = rho(d, distance_static, scale, alpha)
                swr = np.sum(w * r_)
                terms[p, 0] += 0.5 * lam[0] * swr / n
                out_maps[k, p] = w[None] * v
                err["d"][p, k] = d
                if grad:
                    cA = 0.5 * lam[0] / (n * P)
                    cB = -cA * swr / n if sw >= 1e-6 else 0.0
                    with np.errstate(invalid="ignore", divide="ignore"):
                        gv = np.where(d > 0, cA * w * dr / d, 0.0)[None] * v
                    gD = np.sum(gv * A, 0)
                    if not weight_is_data:
                        gD = gD + (cA * r_ + cB) * (-w / D)
                    g[r] += gD
                    _scatter(g, tg, taps, ray_t, -np.einsum("ji,jhw->ihw", R[tg], gv))
    if any(v > 0 for v in lam[1:]):
        nbrs = np.asarray(neighbor_frames).reshape(-1, 4)
        valid = f64(valid).reshape(P, 2)
        fbar = [np.mean(intr[pairs[:, al], :2]) for al in range(2)]   # torch.mean(focal_length(intrinsics_ref)) over the batch
        for p in range(P):
            for al in range(2):
                r, nm, npl = pairs[p][al], nbrs[p][2 * al], nbrs[p][2 * al + 1]
                px, py, ray = _rays(intr, warp, r, H, W)
                D = depth[r]
                Xr = ray * D[None]
                Xw = np.einsum("ij,jhw->ihw", R[r], Xr) + t[r][:, None, None]
                fm, fp = f64(neighbor_flows[2 * al][p]), f64(neighbor_flows[2 * al + 1][p])
                Sm, taps_m, ray_m = _sample(depth, intr, warp, nm, px + fm[0], py + fm[1])
                Sp, taps_p, ray_p = _sample(depth, intr, warp, npl, px + fp[0], py + fp[1])
                Ym = np.einsum("ij,jhw->ihw", R[nm], Sm) + t[nm][:, None, None]
                Yp = np.einsum("ij,jhw->ihw", R[npl], Sp) + t[npl][:, None, None]
                Xs = np.einsum("ji,jhw->ihw", R[r], Yp + Ym - Xw - t[r][:, None, None])
                w = valid[p, al] * f64(neighbor_masks[2 * al][p]).reshape(H, W) * f64(neighbor_masks[2 * al + 1][p]).reshape(H, W)
                n = max(np.sum(w), 1e-6)
                out_maps[2 + 2 * al, p] = w[None] * (Yp - Xw)
                out_maps[3 + 2 * al, p] = w[None] * (Ym - Xw)
                fx, fy, cx, cy = intr[r]
                X, Y, Z = Xs
                Zr = Xr[2]
                dx, dy = cx - fx * X / Z - px, cy + fy * Y / Z - py
                e_rep = np.sqrt(dx * dx + dy * dy)
                e_dsp = 1.0 / Z - 1.0 / Zr
                pa, qa = np.abs(Zr), np.abs(Z)
                e_rat = lam[3] * np.log(np.minimum(pa, qa) / np.maximum(pa, qa))
                err["e_rep"][p, al], err["e_dsp"][p, al], err["z_gap"][p, al] = e_rep, e_dsp, pa - qa
                mult = (lam[1], lam[2] * fbar[al], 1.0 if lam[3] > 0 else 0.0)
                gs = np.zeros((3, H, W))     # d total / d X_s
                gD = np.zeros((H, W))        # d total / d D_r not through X_s
                for q, e in enumerate((e_rep, e_dsp, e_rat)):
                    if lam[1 + q] <= 0:
                        continue
                    r_, dr = rho(e, distance_smooth, scale, alpha)
                    terms[p, 1 + q] += 0.5 * mult[q] * np.sum(w * r_) / n
                    k = 0.5 * mult[q] / (n * P) * w * dr
                    if q == 0:
                        with np.errstate(invalid="ignore", divide="ignore"):
                            kx, ky = np.where(e > 0, k * dx / e, 0.0) * fx, np.where(e > 0, k * dy / e, 0.0) * fy
                        gs[0] += -kx / Z
                        gs[1] += ky / Z
                        gs[2] += (kx * X - ky * Y) / (Z * Z)
                    elif q == 1:
                        gs[2] += -k / (Z * Z)
                        gD += -k / (D * D)
                    else:
                        sg = np.sign(qa - pa) * lam[3]      # +1 where |X_r.z| < |X_s.z|
                        gs[2] += -k * sg / Z
                        gD += k * sg / D
                if grad:
                    gw = np.einsum("ij,jhw->ihw", R[r], gs)
                    # d X_s / d D_r = -R_r^T R_r ray: the rotation as given (f32-rounded), not assumed orthogonal
                    g[r] += gD - np.sum(gw * np.einsum("ij,jhw->ihw", R[r], ray), 0)
                    _scatter(g, nm, taps_m, ray_m, np.einsum("ji,jhw->ihw", R[nm], gw))
                    _scatter(g, npl, taps_p, ray_p, np.einsum("ji,jhw->ihw", R[npl], gw))
    total = float(np.mean(np.sum(terms, 1)))
    out = (total, {name: terms[:, q].copy() for q, name in enumerate(TERMS) if lam[q] > 0})
    if grad:
        out += (g,)
    if maps:
        out += (out_maps,)
    if samples:
        out += (err,)
    return out


def check_kinks(case):
    """Smallest distance of a weighted sample's errors from their sign kinks: (d, e_rep, |e_dsp|, ||X_r.z| - |X_s.z||); inf for a
    part the case does not have."""
    from tests.sceneflow_cases import case_kwargs
    smooth = case["nbrs"] is not None
    lam = (1.0, 1.0, 1.0, 1.0) if smooth else (1.0, 0.0, 0.0, 0.0)
    err = scene_flow(**case_kwargs(case), lambdas=lam, samples=True)[-1]
    P, H, W = case["P"], case["H"], case["W"]
    ws = np.stack([np.asarray(m).reshape(P, H, W) for m in case["masks"]], 1) != 0
    out = [float(err["d"][ws].min())]
    if smooth:
        nm = [np.asarray(m).reshape(P, H, W) for m in case["nmasks"]]
        wm = np.stack([case["valid"][:, al, None, None] * nm[2 * al] * nm[2 * al + 1] for al in range(2)], 1) != 0
        out += [float(err["e_rep"][wm].min()), float(np.abs(err["e_dsp"][wm]).min()), float(np.abs(err["z_gap"][wm]).min())]
    return tuple(out)


def reference_run(case, distance_static, distance_smooth, scale, alpha, lambdas, dtype="float64"):
    """The REAL reference: SceneFlowLoss.__call__ (loss/scene_flow_loss.py) with torch autograd on the CPU, on a case of
    tests/sceneflow_cases.py laid out as its batches (B = P, N = 6: ref, target and the four neighbours gathered from the frame
    table; N = 2 for a static-only case).  Needs the reference checkout; returns float64 numpy (total, {term: [P]}, d total / d
    depth table [F, H, W], the list of visualisation maps).

    * For any distance but l1 the reference builds its alpha / scale tensors in its global f32 dtype and asserts it: the f64 run
      constructs the loss with l1 and sets robust_dist_static / robust_dist_smooth to the reference's loss.general.lossfun with
      f64 tensors.
    * metadata["warp"] is scaled in place by the reference: every call gets a fresh clone."""
    import types

    import torch
    from tests.reference_residuals import _reference_modules
    _reference_modules()
    from loss.general import lossfun
    from loss.scene_flow_loss import SceneFlowLoss
    td = {"float64": torch.float64, "float32": torch.float32}[dtype]
    lam = [float(v) for v in lambdas]
    f64 = td == torch.float64
    opt = types.SimpleNamespace(distance_type_static="l1" if f64 else distance_static,
                                distance_type_smooth="l1" if f64 else distance_smooth, distance_scale=scale, distance_alpha=alpha,
                                lambda_scene_flow_static=lam[0], lambda_smooth_reprojection=lam[1], lambda_smooth_disparity=lam[2],
                                lambda_smooth_depth_ratio=lam[3], recon="colmap" if case["warp"] is None else "i3d")
    loss = SceneFlowLoss(opt)
    if f64:
        def dist(name):
            a = {"l2": 2.0, "smooth_l1": 1.0, "cauchy": 0.0, "general": float(alpha)}[name]
            a_t, s_t = torch.tensor(a, dtype=td), torch.tensor(float(scale), dtype=td)
            return lambda x: lossfun(x, a_t, s_t)
        if distance_static != "l1":
            loss.robust_dist_static = dist(distance_static)
        if distance_smooth != "l1":
            loss.robust_dist_smooth = dist(distance_smooth)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=td)
    P, H, W = case["P"], case["H"], case["W"]
    frames = case["pairs"] if case["nbrs"] is None else np.concatenate([case["pairs"], case["nbrs"]], 1)
    idx = torch.tensor(np.asarray(frames, np.int64))
    table = t(case["depth"]).requires_grad_(True)
    meta = {"extrinsics": t(case["extrinsics"])[idx], "intrinsics": t(case["intrinsics"])[idx],
            "geometry_consistency": {"flows": tuple(t(f) for f in case["flows"]),
                                     "masks": tuple(t(m).view(P, 1, H, W) for m in case["masks"])}}
    if case["nbrs"] is not None:
        meta["temporal_smoothness"] = {"flows": tuple(t(f) for f in case["nflows"]),
                                       "masks": tuple(t(m).view(P, 1, H, W) for m in case["nmasks"]),
                                       "valid": t(case["valid"]).view(P, 2, 1)}
    if case["warp"] is not None:
        meta["warp"] = t(case["warp_norm"])[idx].clone()
    total, batch, maps = loss(table[idx], meta)
    total.backward()
    terms = {name: batch[name].detach().double().numpy().copy() for q, name in enumerate(TERMS) if lam[q] > 0}
    return float(total.detach().double()), terms, table.grad.double().numpy().copy(), [np.asarray(m, np.float64) for m in maps]
