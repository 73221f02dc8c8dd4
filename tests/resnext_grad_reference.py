"""float64 numpy restatement, from the definitions, of the backbone's training operators for
robust_cvd_amd/csrc/cvd_resnext_grad.h: nn.BatchNorm2d in training and eval mode and its backward, the gradients of the (grouped,
strided) convolutions and of nn.MaxPool2d(3, 2, 1) with torch's first-maximum rule.  The mathematics in double, from the f32 inputs.
The fixture (resnext_grad_golden.npz, minted by tests/golden/reference_py/make_resnext_grad_golden.py from stock torch autograd on
the CPU; never from the kernels) records how far torch's f32 arithmetic is from it.  numpy only."""
import os

import numpy as np

from tests import resnext_cases as rc
from tests import resnext_grad_cases as gc
from tests import resnext_reference as rr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "resnext_grad_golden.npz")
bar = rr.bar
STORED_ELEMENTS = 4096                  # torch's f32 tensors up to this size are stored in the fixture; of larger ones delta and scale


def norm_train(c, norm, eps=gc.EPS, momentum=gc.MOMENTUM, training=True, relu=False, residual=None):
    """-> (y, save_mean, save_invstd, running_mean, running_var) as torch's batch_norm forms them."""
    c = np.asarray(c, np.float64)
    gamma, beta, rmean, rvar = (np.asarray(v, np.float64) for v in norm)
    M = c.shape[0] * c.shape[2] * c.shape[3]
    if training:
        mean = c.mean(axis=(0, 2, 3))
        var = ((c - mean[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
        rmean = (1 - momentum) * rmean + momentum * mean
        rvar = (1 - momentum) * rvar + momentum * var * M / (M - 1)
    else:
        mean, var = rmean, rvar
    invstd = 1.0 / np.sqrt(var + eps)
    y = (c - mean[None, :, None, None]) * (invstd * gamma)[None, :, None, None] + beta[None, :, None, None]
    if relu:
        y = np.maximum(y, 0)
    if residual is not None:
        y = np.maximum(y + np.asarray(residual, np.float64), 0)
    return y, mean, invstd, rmean, rvar


def norm_grad(gy, c, mean, invstd, gamma, y=None, training=True):
    """-> (gc, g_gamma, g_beta, g): g = gy where y > 0 (all of gy without y)."""
    gy, c = np.asarray(gy, np.float64), np.asarray(c, np.float64)
    mean, invstd, gamma = (np.asarray(v, np.float64)[None, :, None, None] for v in (mean, invstd, gamma))
    g = gy if y is None else np.where(np.asarray(y) > 0, gy, 0.0)
    xhat = (c - mean) * invstd
    M = c.shape[0] * c.shape[2] * c.shape[3]
    gb, gg = g.sum(axis=(0, 2, 3)), (g * xhat).sum(axis=(0, 2, 3))
    if training:
        out = gamma * invstd * (g - gb[None, :, None, None] / M - xhat * gg[None, :, None, None] / M)
    else:
        out = g * gamma * invstd
    return out, gg, gb, g


def conv_grads(gy, x, weight, stride, groups):
    """(gx, gW) of nn.Conv2d(Cin, N, k, stride, padding=k // 2, groups=groups, bias=False): sums over the taps of the definition."""
    gy, x, weight = (np.asarray(v, np.float64) for v in (gy, x, weight))
    B, Cin, H, W = x.shape
    N, cg, k, _ = weight.shape
    ng, pad = N // groups, k // 2
    Ho, Wo = gy.shape[2:]
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    gxp = np.zeros_like(xp)
    gw = np.zeros_like(weight)
    for g in range(groups):
        gyg, wg = gy[:, g * ng:(g + 1) * ng], weight[g * ng:(g + 1) * ng]
        for i in range(k):
            for j in range(k):
                rows, cols = slice(i, i + stride * (Ho - 1) + 1, stride), slice(j, j + stride * (Wo - 1) + 1, stride)
                gw[g * ng:(g + 1) * ng, :, i, j] = np.einsum("bnyx,bcyx->nc", gyg, xp[:, g * cg:(g + 1) * cg, rows, cols])
                gxp[:, g * cg:(g + 1) * cg, rows, cols] += np.einsum("bnyx,nc->bcyx", gyg, wg[:, :, i, j])
    return gxp[:, :, pad:pad + H, pad:pad + W], gw


def maxpool_grad(x, gy):
    """Backward of nn.MaxPool2d(3, 2, 1): each window's gradient to its FIRST maximum in row-major order, padding excluded."""
    x, gy = np.asarray(x), np.asarray(gy, np.float64)
    B, Cn, H, W = x.shape
    Ho, Wo = gy.shape[2:]
    gx = np.zeros(x.shape, np.float64)
    for oy in range(Ho):
        for ox in range(Wo):
            ys = [y for y in range(2 * oy - 1, 2 * oy + 2) if 0 <= y < H]
            xs = [v for v in range(2 * ox - 1, 2 * ox + 2) if 0 <= v < W]
            window = x[:, :, ys][:, :, :, xs].reshape(B, Cn, -1)
            arg = window.argmax(axis=2)                           # numpy's argmax is the first maximum
            for b in range(B):
                for ch in range(Cn):
                    gx[b, ch, ys[arg[b, ch] // len(xs)], xs[arg[b, ch] % len(xs)]] += gy[b, ch, oy, ox]
    return gx


def norm_case(case):
    """-> forward tuple of norm_train and backward tuple (gc, g_gamma, g_beta, g_residual) of the case."""
    fwd = norm_train(case["c"], case["norm"], training=case["training"], relu=case["relu"], residual=case["residual"])
    masked = case["relu"] or case["residual"] is not None
    y32 = fwd[0].astype(np.float32)
    bwd = norm_grad(case["gy"], case["c"], fwd[1], fwd[2], case["norm"][0], y32 if masked else None, case["training"])
    return fwd, bwd


def grouped_case(case):
    return conv_grads(case["gy"], case["x"], case["weight"], case["stride"], case["groups"])


def dense_case(case):
    gx, gw = conv_grads(case["gy"], case["x"], case["weight"], case["stride"], 1)
    return (gx if case["add"] is None else gx + case["add"]), gw


def conv_forward(x, weight, stride, groups):
    return rr.conv2d(x, weight, stride) if groups == 1 else rr.grouped_conv2d(x, weight, stride, groups)


def block_case(case):
    """One Bottleneck forward and backward, chained from the definitions above -> {name: f64 array}: out, gx, per convolution i
    gw{i}, gg{i}, gb{i} and, in training mode, rm{i}, rv{i} (the running statistics after the forward)."""
    x, ws, norms, stride, groups, tr = case["x"], case["weights"], case["norms"], case["stride"], case["groups"], case["training"]
    down = len(ws) == 4
    c1 = conv_forward(x, ws[0], 1, 1)
    f1 = norm_train(c1, norms[0], training=tr, relu=True)
    c2 = conv_forward(f1[0], ws[1], stride, groups)
    f2 = norm_train(c2, norms[1], training=tr, relu=True)
    identity, fd = np.asarray(x, np.float64), None
    if down:
        cd = conv_forward(x, ws[3], stride, 1)
        fd = norm_train(cd, norms[3], training=tr)
        identity = fd[0]
    c3 = conv_forward(f2[0], ws[2], 1, 1)
    f3 = norm_train(c3, norms[2], training=tr, residual=identity)
    out = {"out": f3[0]}
    gc3, gg3, gb3, gres = norm_grad(case["gy"], c3, f3[1], f3[2], norms[2][0], f3[0], tr)
    g2, gw3 = conv_grads(gc3, f2[0], ws[2], 1, 1)
    gc2, gg2, gb2, _ = norm_grad(g2, c2, f2[1], f2[2], norms[1][0], f2[0], tr)
    g1, gw2 = conv_grads(gc2, f1[0], ws[1], stride, groups)
    gc1, gg1, gb1, _ = norm_grad(g1, c1, f1[1], f1[2], norms[0][0], f1[0], tr)
    gx, gw1 = conv_grads(gc1, x, ws[0], 1, 1)
    grads = [(gw1, gg1, gb1), (gw2, gg2, gb2), (gw3, gg3, gb3)]
    if down:
        gcd, ggd, gbd, _ = norm_grad(gres, cd, fd[1], fd[2], norms[3][0], None, tr)
        gxd, gwd = conv_grads(gcd, x, ws[3], stride, 1)
        grads.append((gwd, ggd, gbd))
        gx = gx + gxd
    else:
        gx = gx + gres
    out["gx"] = gx
    for i, (gw, gg, gb) in enumerate(grads):
        out.update({f"gw{i}": gw, f"gg{i}": gg, f"gb{i}": gb})
    if tr:
        for i, f in enumerate([f1, f2, f3] + ([fd] if down else [])):
            out.update({f"rm{i}": f[3], f"rv{i}": f[4]})
    return out
