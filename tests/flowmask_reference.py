"""Numpy restatement of the flow consistency masks (the reference's Flow.compute_flow_masks, flow.py:180-209, and
utils/consistency.py:8-67), written from the definition in DESIGN.md §3.9; the errors are formed in float64.

Direction a -> b of a pair, pixel (x, y) with integer coordinates:
  1. target tx = x + Fab[y, x, 0], ty = y + Fab[y, x, 1] in f64; in bounds iff 0 <= tx <= W - 1 and 0 <= ty <= H - 1
  2. gx = f32(2 tx / W - 1), gy = f32(2 ty / H - 1): the ONE f32 rounding that is kept, because it moves the sampling position;
     px = ((gx + 1) W - 1) / 2 = tx - 0.5 clamped to [0, W - 1] (NaN -> 0), likewise py; bilinear taps floor(px), floor(px) + 1;
     a tap outside the image contributes 0 (only the +1 tap at the last column / row, whose weight is 0)
  3. ef = sum_c (Fab[c] + S(Fba)[c])^2, ec = sum_c (Ca[c] - S(Cb)[c])^2
  4. mask = in bounds and ef < f32(flow_thresh^2) and ec < f32(C color_thresh^2); a NaN fails a comparison
"""
import numpy as np


def thresholds(flow_thresh, color_thresh, channels):
    """The two f32 thresholds: formed in double from the (f32) arguments of the C ABI, rounded once."""
    ft, ct = float(np.float32(flow_thresh)), float(np.float32(color_thresh))
    return np.float32(ft * ft), np.float32(channels * (ct * ct))


def sample_positions(flow):
    """(tx, ty) f64 targets, in-bounds flags and the clamped f64 sampling positions (px, py) of a flow image [H, W, 2]."""
    H, W = flow.shape[:2]
    x, y = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    tx, ty = x + flow[..., 0].astype(np.float64), y + flow[..., 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        inb = (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
        gx = (2.0 * tx / W - 1.0).astype(np.float32).astype(np.float64)
        gy = (2.0 * ty / H - 1.0).astype(np.float32).astype(np.float64)
        px, py = ((gx + 1.0) * W - 1.0) / 2.0, ((gy + 1.0) * H - 1.0) / 2.0
        px = np.where(np.isnan(px), 0.0, np.clip(px, 0.0, W - 1.0))
        py = np.where(np.isnan(py), 0.0, np.clip(py, 0.0, H - 1.0))
    return tx, ty, inb, px, py


def bilinear(img, px, py):
    """img [H, W, K] sampled at the clamped positions: [H, W, K] f64."""
    H, W = img.shape[:2]
    img = img.reshape(H, W, -1).astype(np.float64)
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    wx, wy = (px - x0)[..., None], (py - y0)[..., None]
    xin, yin = (x0 + 1 < W)[..., None], (y0 + 1 < H)[..., None]
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    with np.errstate(invalid="ignore"):
        return (img[y0, x0] * ((1 - wy) * (1 - wx)) + np.where(xin, img[y0, x1], 0.0) * ((1 - wy) * wx)
                + np.where(yin, img[y1, x0], 0.0) * (wy * (1 - wx)) + np.where(xin & yin, img[y1, x1], 0.0) * (wy * wx))


def direction_errors(flow_own, flow_other, color_own, color_other):
    """(in bounds [H, W] bool, ef [H, W] f64, ec [H, W] f64) of one direction."""
    H, W = flow_own.shape[:2]
    _tx, _ty, inb, px, py = sample_positions(flow_own)
    with np.errstate(invalid="ignore", over="ignore"):
        df = flow_own.astype(np.float64) + bilinear(flow_other, px, py)
        dc = color_own.reshape(H, W, -1).astype(np.float64) - bilinear(color_other, px, py)
        return inb, np.sum(df * df, axis=-1), np.sum(dc * dc, axis=-1)


def direction_mask(flow_own, flow_other, color_own, color_other, flow_thresh=1.0, color_thresh=1.0):
    """uint8 [H, W] mask (255 / 0) of one direction."""
    channels = color_own.reshape(flow_own.shape[0], flow_own.shape[1], -1).shape[-1]
    tf, tc = thresholds(flow_thresh, color_thresh, channels)
    inb, ef, ec = direction_errors(flow_own, flow_other, color_own, color_other)
    with np.errstate(invalid="ignore"):
        keep = inb & (ef < float(tf)) & (ec < float(tc))
    return np.where(keep, 255, 0).astype(np.uint8)


def pair_masks(flow_ab, flow_ba, color_a, color_b, flow_thresh=1.0, color_thresh=1.0):
    """(mask_ab, mask_ba) of one pair."""
    return (direction_mask(flow_ab, flow_ba, color_a, color_b, flow_thresh, color_thresh),
            direction_mask(flow_ba, flow_ab, color_b, color_a, flow_thresh, color_thresh))


def batch(color, pairs, flow_ab, flow_ba, flow_thresh=1.0, color_thresh=1.0):
    """What Solver.flow_consistency_masks(..., return_errors=True) returns, in f64: (mask_ab [P, H, W], mask_ba, kept [P, 2],
    errors [P, 2, H, W, 2])."""
    P, H, W = flow_ab.shape[:3]
    channels = color.shape[-1]
    tf, tc = thresholds(flow_thresh, color_thresh, channels)
    mab, mba = np.zeros((P, H, W), np.uint8), np.zeros((P, H, W), np.uint8)
    err = np.zeros((P, 2, H, W, 2), np.float64)
    for p, (a, b) in enumerate(np.asarray(pairs).tolist()):
        for d, (fo, ft, co, ctg, out) in enumerate(((flow_ab[p], flow_ba[p], color[a], color[b], mab),
                                                     (flow_ba[p], flow_ab[p], color[b], color[a], mba))):
            inb, ef, ec = direction_errors(fo, ft, co, ctg)
            with np.errstate(invalid="ignore"):
                out[p] = np.where(inb & (ef < float(tf)) & (ec < float(tc)), 255, 0)
            err[p, d, ..., 0], err[p, d, ..., 1] = ef, ec
    kept = np.stack([(mab > 0).sum(axis=(1, 2)), (mba > 0).sum(axis=(1, 2))], axis=1).astype(np.int32)
    return mab, mba, kept, err


# ---- the reference's own functions (golden minting and the live CPU test; never on the GPU box) -----------------------
BAND = 8.0          # undecided: |e - threshold| <= BAND * delta, delta = max |e_ref32 - e_f64| measured when the golden is minted
SMALL = 10.0        # errors below are compared absolutely (delta), the others relatively (delta_rel)
MAX_UNDECIDED = 1e-3


def load_reference_consistency():
    """The reference's utils/consistency.py as a module, or None when the reference (or torch) is not on this machine."""
    import importlib.util
    import os
    root = os.environ.get("ROBUST_CVD_REFERENCE", "/root/reference")
    path = os.path.join(root, "utils", "consistency.py")
    if not os.path.isfile(path):
        return None
    try:
        import torch  # noqa: F401
    except Exception:
        return None
    spec = importlib.util.spec_from_file_location("reference_utils_consistency", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_pair(cons, flow_ab, flow_ba, color_a, color_b, flow_thresh, color_thresh):
    """The reference's masks of one pair (consistent_flow_masks) and its own f32 error maps (sample + sse):
    (masks [2, H, W] bool, errors [2, H, W, 2] f32)."""
    H, W = flow_ab.shape[:2]
    flows, colors = [flow_ab, flow_ba], [color_a, color_b]
    with np.errstate(invalid="ignore"):
        masks = np.stack(cons.consistent_flow_masks(flows, colors, flow_thresh, color_thresh))
        err = np.zeros((2, H, W, 2), np.float32)
        X, Y = np.meshgrid(np.arange(W), np.arange(H))
        for d, (fo, ft, co, ct) in enumerate(((flow_ab, flow_ba, color_a, color_b), (flow_ba, flow_ab, color_b, color_a))):
            uv = np.stack((fo[..., 0] + X, fo[..., 1] + Y), axis=-1)
            err[d, ..., 0] = cons.sse(fo, cons.sample(-ft, uv))
            err[d, ..., 1] = cons.sse(co, cons.sample(ct, uv))
    return masks.astype(bool), err


def deltas(err_ref32, err_f64):
    """(delta, delta_rel): max |e_ref32 - e_f64| over finite errors with e_ref32 < SMALL, max relative difference over the rest."""
    a, b = err_ref32.astype(np.float64).ravel(), err_f64.ravel()
    fin = np.isfinite(a) & np.isfinite(b)
    small = fin & (a < SMALL)
    big = fin & ~small
    d = float(np.abs(a[small] - b[small]).max()) if small.any() else 0.0
    dr = float((np.abs(a[big] - b[big]) / np.abs(b[big])).max()) if big.any() else 0.0
    return d, dr


def undecided(err_ref32, delta, flow_thresh, color_thresh, channels):
    """[..., H, W] bool: pixels whose reference error lies within BAND * delta of its threshold, for either error."""
    tf, tc = thresholds(flow_thresh, color_thresh, channels)
    e = err_ref32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (np.abs(e[..., 0] - float(tf)) <= BAND * delta) | (np.abs(e[..., 1] - float(tc)) <= BAND * delta)


def errors_close(err, err_ref32, delta, delta_rel):
    """[...] bool per value: within BAND * delta absolutely where the reference's error is < SMALL, within BAND * delta_rel
    relatively elsewhere; a non-finite reference value asks for the same non-finite value."""
    a, b = np.asarray(err, np.float64), err_ref32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(b)
        ok_small = np.abs(a - b) <= BAND * delta
        ok_big = np.abs(a - b) <= BAND * delta_rel * np.abs(b)
        same = (np.isnan(a) & np.isnan(b)) | (a == b)
        return np.where(fin, np.where(b < SMALL, ok_small, ok_big), same)
