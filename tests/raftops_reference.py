"""float64 numpy restatement of the three RAFT operators of robust_cvd_amd/csrc/cvd_raftops.h: the correlation pyramid and its
windowed lookup (reference raft/core/corr.py:8-46 with raft/core/utils/utils.py:56-70) and the convex upsampling
(raft/core/raft.py:49-60).  The mathematics in double, from the f32 inputs; the fixture (raftops_golden.npz, minted by
tests/golden/reference_py/make_raftops_golden.py) records how far the reference's own f32 arithmetic is from it."""
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "raftops_golden.npz")
EPS32 = 2.0 ** -23


def level0_f32(raw, dim):
    """Level 0 as torch and numpy round it: an f32 division by the f32 square root of dim."""
    return raw / np.float32(np.sqrt(np.float32(dim)))


def pyramid(raw, dim, levels):
    """raw [Q, h, w] -> list of `levels` f64 arrays; level l + 1 = 2 x 2 means of level l, an odd last row / column dropped."""
    out = [raw.astype(np.float64) / np.float64(np.float32(np.sqrt(np.float32(dim))))]
    for _ in range(levels - 1):
        a = out[-1]
        h, w = a.shape[1] // 2, a.shape[2] // 2
        a = a[:, :2 * h, :2 * w]
        out.append((a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]) / 4.0)
    return out


def _sample_zero_padded(vol, x, y):
    """Bilinear samples of vol [Q, h, w] at x, y [Q, ...] (pixel centres at integers, corners by floor, corners outside count 0)."""
    Q, h, w = vol.shape
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    qi = np.arange(Q).reshape((Q,) + (1,) * (x.ndim - 1))
    out = np.zeros(x.shape, np.float64)
    for dy, wy in ((0, 1.0 - fy), (1, fy)):
        for dx, wx in ((0, 1.0 - fx), (1, fx)):
            cx, cy = x0 + dx, y0 + dy
            inside = (cx >= 0) & (cx <= w - 1) & (cy >= 0) & (cy <= h - 1)
            ix = np.where(inside, cx, 0).astype(np.int64)
            iy = np.where(inside, cy, 0).astype(np.int64)
            out += np.where(inside, vol[qi, iy, ix] * wx * wy, 0.0)
    return out


def lookup(levels_list, coords, radius):
    """levels_list: arrays [Q, h_l, w_l]; coords [B, 2, h1, w1] (channel 0 = x) -> [B, L n^2, h1, w1] f64, n = 2 radius + 1, channel
    l n^2 + a n + b sampling level l at (x / 2^l + a - radius, y / 2^l + b - radius): the first window index moves x."""
    B, _, h1, w1 = coords.shape
    n = 2 * radius + 1
    c = coords.astype(np.float64)
    cx, cy = c[:, 0].reshape(-1, 1, 1), c[:, 1].reshape(-1, 1, 1)
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    out = []
    for l, vol in enumerate(levels_list):
        x = cx / 2.0 ** l + d.reshape(1, n, 1) + np.zeros((1, 1, n))
        y = cy / 2.0 ** l + d.reshape(1, 1, n) + np.zeros((1, n, 1))
        out.append(_sample_zero_padded(np.asarray(vol, np.float64), x, y).reshape(B, h1, w1, n * n))
    return np.ascontiguousarray(np.concatenate(out, -1).transpose(0, 3, 1, 2))


def upsample(flow, mask):
    """flow [N, 2, H, W], mask [N, 576, H, W] -> [N, 2, 8 H, 8 W] f64."""
    N, _, H, W = flow.shape
    m = mask.astype(np.float64).reshape(N, 9, 8, 8, H, W)
    m = np.exp(m - m.max(1, keepdims=True))
    m /= m.sum(1, keepdims=True)
    f = np.zeros((N, 2, H + 2, W + 2), np.float64)
    f[:, :, 1:-1, 1:-1] = 8.0 * flow.astype(np.float64)
    nb = np.stack([f[:, :, k // 3:k // 3 + H, k % 3:k % 3 + W] for k in range(9)], 2)     # [N, 2, 9, H, W]
    up = np.einsum("nkijyx,nckyx->ncyixj", m, nb)
    return np.ascontiguousarray(up.reshape(N, 2, 8 * H, 8 * W))


def bar(delta, scale):
    """The suite's bar of an f32 kernel against the f64 restatement: 8 x the reference's own f32 error for the case (never below
    one f32 ulp of the output scale)."""
    return 8.0 * max(float(delta), EPS32 * float(scale))


def load_reference():
    """(CorrBlock, upsample_flow) of the reference checkout (ROBUST_CVD_REFERENCE, default /root/reference) on CPU tensors, or
    None where it (or torch) is not available."""
    root = os.environ.get("ROBUST_CVD_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(root, "raft", "core", "corr.py")):
        return None
    try:
        import torch  # noqa: F401
    except ImportError:
        return None
    added = root not in sys.path
    if added:
        sys.path.insert(0, root)
    try:
        from raft.core.corr import CorrBlock
        from raft.core.raft import RAFT
    finally:
        if added:
            sys.path.remove(root)
    return CorrBlock, lambda flow, mask: RAFT.upsample_flow(None, flow, mask)


def reference_outputs(ref, case):
    """The reference's f32 results for a correlation case: (pyramid levels [Q, h_l, w_l], lookup [B, C, h, w])."""
    import torch
    CorrBlock = ref[0]
    with torch.no_grad():
        block = CorrBlock(torch.from_numpy(case["fmap1"]), torch.from_numpy(case["fmap2"]), num_levels=case["levels"],
                          radius=case["r"])
        out = block(torch.from_numpy(case["coords"]))
    return [t[:, 0].numpy() for t in block.corr_pyramid], out.numpy()


def reference_upsample(ref, case):
    import torch
    with torch.no_grad():
        return ref[1](torch.from_numpy(case["flow"]), torch.from_numpy(case["mask"])).numpy()
