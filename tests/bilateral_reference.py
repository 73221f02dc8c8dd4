"""numpy restatement of DepthVideoProcessor::bilateralFilter, reference lib/Processor.cpp:183-313 (defaults
lib/Processor.h:64-70), f32 and order-faithful:

- the mean loops over the window offsets (frame ascending, then row, then column: :262-292) and accumulates whole arrays
  elementwise, which keeps every pixel's own accumulation order;
- exp is taken in f64 and rounded to f32 (the reference's expf, :285, correctly rounded up to glibc's last bit);
- the median sorts each pixel's (depth, weight) pairs lexicographically (std::sort of std::pair, :297) and takes the first
  sample whose running f32 weight sum reaches half the total (:294-306);
- in place (depthStream 0, the default) the frames are filtered in ascending order and each written frame is passed through
  a per-frame transform callback before later windows read it (setDepth replaces the source, depth() re-applies the
  transform: :311, DepthStream.cpp:102-116).
"""
import numpy as np

F32 = np.float32


def _exp32(e):
    return np.exp(e.astype(np.float64)).astype(F32)


def _weights(d, dref, c, cref, depth_sigma, color_sigma):
    """:268-285; d / dref [h][w] f32, c / cref [h][w][3] f32 (ignored when color_sigma <= 0)."""
    exponent = np.zeros(d.shape, F32)
    if depth_sigma > 0:                                   # :266-270
        s2 = F32(depth_sigma) * F32(depth_sigma)          # sqr(params.depthSigma), :184
        diff = (d - dref).astype(F32)
        exponent = (exponent + (-(diff * diff)) / s2).astype(F32)
    if color_sigma > 0:                                   # :272-279
        s2 = F32(color_sigma) * F32(color_sigma)
        e = (c - cref).astype(F32)
        diff2 = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).astype(F32)
        exponent = (exponent + (-diff2) / s2).astype(F32)
    return np.where(exponent != 0, _exp32(exponent), F32(1)).astype(F32)  # :281


def _window(n, f, h, w, frame_radius, spatial_radius):
    """(frames, [(dy, dx)]) of the window of frame f in the reference's order (:211-213, :230-242)."""
    f0, f1 = max(0, f - frame_radius), min(n - 1, f + frame_radius)
    r = spatial_radius
    return range(f0, f1 + 1), [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]


def _shifted(img, dy, dx, fill):
    """img[y + dy, x + dx] for every (y, x), `fill` where that lies outside the image; and the validity mask."""
    h, w = img.shape[:2]
    out = np.full(img.shape, fill, dtype=img.dtype)
    valid = np.zeros((h, w), bool)
    ys, yd = slice(max(0, dy), min(h, h + dy)), slice(max(0, -dy), min(h, h - dy))
    xs, xd = slice(max(0, dx), min(w, w + dx)), slice(max(0, -dx), min(w, w - dx))
    out[yd, xd] = img[ys, xs]
    valid[yd, xd] = True
    return out, valid


def filter_frame(depth, color, f, frame_radius, spatial_radius=0, depth_sigma=0.3, color_sigma=0.0, median=False):
    """Filtered depth of frame f of the batch: depth [n][h][w] f32 (transformed), color [n][h][w][3] f32 BGR or None."""
    depth = np.asarray(depth, F32)
    n, h, w = depth.shape
    color = np.zeros((n, h, w, 3), F32) if color is None else np.asarray(color, F32)
    dref, cref = depth[f], color[f]
    frames, offsets = _window(n, f, h, w, frame_radius, spatial_radius)
    sum_depth = np.zeros((h, w), F32)
    sum_weight = np.zeros((h, w), F32)
    ds, ws, vs = [], [], []
    for k in frames:
        for dy, dx in offsets:
            d, valid = _shifted(depth[k], dy, dx, F32(0))
            c, _ = _shifted(color[k], dy, dx, F32(0))
            wgt = _weights(d, dref, c, cref, depth_sigma, color_sigma)
            if median:
                ds.append(d)
                ws.append(wgt)
                vs.append(valid)
            else:
                sum_depth = np.where(valid, sum_depth + d * wgt, sum_depth).astype(F32)  # :287-289
            sum_weight = np.where(valid, sum_weight + wgt, sum_weight).astype(F32)    # :290
    if not median:
        return np.where(sum_weight > 0, sum_depth / np.where(sum_weight > 0, sum_weight, F32(1)), F32(0)).astype(F32)
    D, W, V = np.stack(ds, -1), np.stack(ws, -1), np.stack(vs, -1)
    half = (sum_weight / F32(2)).astype(F32)
    out = np.zeros((h, w), F32)
    for y in range(h):
        for x in range(w):
            d, wgt = D[y, x][V[y, x]], W[y, x][V[y, x]]
            order = np.lexsort((wgt, d))   # std::pair order: depth, then weight
            cum = F32(0)
            for i in order:
                cum = F32(cum + wgt[i])
                if cum >= half[y, x]:
                    out[y, x] = d[i]
                    break
    return out


def bilateral_filter(depth, color, frame_radius, spatial_radius=0, depth_sigma=0.3, color_sigma=0.0, median=False,
                     first=0, count=None):
    """Out of place: frames [first, first + count) of the batch, every window reading the unfiltered input."""
    n = np.asarray(depth).shape[0]
    count = n - first if count is None else count
    return np.stack([filter_frame(depth, color, f, frame_radius, spatial_radius, depth_sigma, color_sigma, median)
                     for f in range(first, first + count)])


def bilateral_filter_in_place(depth, color, frames, frame_radius, transform, spatial_radius=0, depth_sigma=0.3,
                              color_sigma=0.0, median=False):
    """In place (depthStream == source stream 0): `depth` holds depth() of every video frame; the frames are filtered in
    ascending order, the filtered source of frame f is stored and depth() of f becomes transform(f, filtered).  Returns
    (sources written {f: filtered}, depth() of every frame afterwards)."""
    cur = np.array(depth, F32, copy=True)
    written = {}
    for f in sorted(frames):
        filtered = filter_frame(cur, color, f, frame_radius, spatial_radius, depth_sigma, color_sigma, median)
        written[f] = filtered
        cur[f] = np.asarray(transform(f, filtered), F32)
    return written, cur
