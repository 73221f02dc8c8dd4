"""float64 numpy restatement of the backward of the MiDaS decoder's layers for robust_cvd_amd/csrc/cvd_midas_grad.h: the gradients
torch's autograd computes for the reference's nn.Conv2d(stride 1, padding k // 2) (monodepth/midas_v2/blocks.py:39-50, 100-107;
midas_net.py:36-40) and for its bilinear x 2 interpolate (blocks.py:54-84, 155-157), and the bar of the GPU tests.  The mathematics in
double from the f32 inputs, written from the DEFINITIONS (a scatter for the input gradient, a correlation for the weight gradient, the
transposed interpolation matrices), not from the kernels' scheme.  The masks of the operator cases are given f32 tensors: exact.  The
fixture (midas_grad_golden.npz, minted by tests/golden/reference_py/make_midas_grad_golden.py under torch's autograd on the CPU)
records how far torch's f32 arithmetic is from it.  numpy only."""
import os

import numpy as np

from tests import midas_reference as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "midas_grad_golden.npz")
EPS32 = mr.EPS32
bar = mr.bar


def conv_grad_input(gy, weight, add=None, mask=None):
    """gx[b][c][h][w] = sum_{n,i,j} gy[b][n][h - i + p][w - j + p] W[n][c][i][j]; + add; zero where mask <= 0."""
    gy, weight = np.asarray(gy, np.float64), np.asarray(weight, np.float64)
    B, N, H, W = gy.shape
    N2, C, k, k2 = weight.shape
    assert N == N2 and k == k2 and k % 2 == 1
    p = k // 2
    padded = np.zeros((B, C, H + 2 * p, W + 2 * p))
    for i in range(k):
        for j in range(k):
            # output pixel (h, w) read input (h + i - p, w + j - p) with W[:, :, i, j]: its gradient goes back there
            padded[:, :, i:i + H, j:j + W] += np.einsum("bnhw,nc->bchw", gy, weight[:, :, i, j])
    gx = padded[:, :, p:p + H, p:p + W]
    if add is not None:
        gx = gx + np.asarray(add, np.float64)
    if mask is not None:
        gx = np.where(np.asarray(mask) > 0, gx, 0.0)
    return gx


def conv_grad_weight(gy, x, k, relu_in=False):
    """(gW[n][c][i][j] = sum_{b,h,w} gy[b][n][h][w] X[b][c][h + i - p][w + j - p], gbias[n] = sum gy[b][n][h][w])."""
    gy, x = np.asarray(gy, np.float64), np.asarray(x, np.float64)
    if relu_in:
        x = np.maximum(x, 0.0)
    B, N, H, W = gy.shape
    C = x.shape[1]
    p = k // 2
    padded = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
    gw = np.empty((N, C, k, k))
    flat = gy.transpose(1, 0, 2, 3).reshape(N, B * H * W)
    for i in range(k):
        for j in range(k):
            gw[:, :, i, j] = flat @ padded[:, :, i:i + H, j:j + W].transpose(0, 2, 3, 1).reshape(B * H * W, C)
    return gw, flat.sum(axis=1)


def conv_forward(x, weight, relu_in=False):
    """The convolution these are the gradients of (no bias), for the adjoint identities."""
    return mr.conv2d(mr.relu(x) if relu_in else x, weight)


def upsample_matrix(n, align_corners):
    """[2 n, n]: the interpolation along one axis as tests/midas_reference.py: upsample2x forms it."""
    d = np.arange(2 * n, dtype=np.float64)
    if align_corners:
        src = d * ((n - 1) / (2 * n - 1)) if 2 * n > 1 else 0.0 * d
    else:
        src = np.maximum((d + 0.5) * 0.5 - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = src - i0
    A = np.zeros((2 * n, n))
    np.add.at(A, (np.arange(2 * n), i0), 1.0 - l1)
    np.add.at(A, (np.arange(2 * n), i1), l1)
    return A


def upsample2x_grad(gy, align_corners):
    """gy [.., 2 H, 2 W] -> gx [.., H, W] = Ay^T gy Ax."""
    gy = np.asarray(gy, np.float64)
    H, W = gy.shape[-2] // 2, gy.shape[-1] // 2
    return np.einsum("yh,...yx,xw->...hw", upsample_matrix(H, align_corners), gy, upsample_matrix(W, align_corners))


def conv_grad_case(case):
    """{gx, gw, gb} of a case of tests/midas_grad_cases.py."""
    gw, gb = conv_grad_weight(case["gy"], case["x"], case["k"], case["relu_in"])
    return {"gx": conv_grad_input(case["gy"], case["weight"], case["add"], case["mask"]), "gw": gw, "gb": gb}


def upsample_grad_case(case):
    return {"gx": upsample2x_grad(case["gy"], case["align_corners"])}


def head_forward(case):
    """(t, s) of the head in f64: t = output_conv.2(x) + bias2 [B, 32, H, W], s = output_conv.4(relu(t)) + bias4 [B, H, W], the
    output before the last ReLU."""
    t = mr.conv2d(case["x"], case["weight2"], case["bias2"])
    s = mr.conv2d(mr.relu(t), case["weight4"], case["bias4"])[:, 0]
    return t, s


def head_grad_case(case):
    """{gx, gw2, gb2, gw4, gb4}: the masks from the f64 forward."""
    t, s = head_forward(case)
    gs = np.asarray(case["gy"], np.float64)
    if case["non_negative"]:
        gs = np.where(s > 0, gs, 0.0)
    w4 = np.asarray(case["weight4"], np.float64).reshape(1, -1, 1, 1)
    g32 = np.where(t > 0, gs[:, None] * w4, 0.0)
    gw2, gb2 = conv_grad_weight(g32, case["x"], 3)
    return {"gx": conv_grad_input(g32, case["weight2"]), "gw2": gw2, "gb2": gb2,
            "gw4": (gs[:, None] * mr.relu(t)).sum(axis=(0, 2, 3)).reshape(case["weight4"].shape), "gb4": gs.sum().reshape(1)}


def unit_backward(g, x, t1, weights):
    """Backward of conv2(relu(conv1(relu(x)))) + relu(x) at output gradient g; t1 = conv1's result.  -> (gx, gw1, gb1, gw2, gb2)."""
    gw2, gb2 = conv_grad_weight(g, t1, 3, True)
    g1 = conv_grad_input(g, weights[1], mask=t1)
    gw1, gb1 = conv_grad_weight(g1, x, 3, True)
    return conv_grad_input(g1, weights[0], add=g, mask=x), gw1, gb1, gw2, gb2


def decoder_forward(case):
    """The decoder of tests/midas_reference.py: decoder, keeping what the backward reads: {rn, t1, o, t2 per level, p0, h0, hup, t, s}
    (level 3 has no t1; its o is rn[3])."""
    p, maps = case["params"], case["maps"]
    rn = [mr.conv2d(m, p[f"layer{k + 1}_rn"][0]) for k, m in enumerate(maps)]
    t1, o, t2 = [None] * 4, [None] * 4, [None] * 4
    path = None
    for k in (3, 2, 1, 0):
        name = f"refinenet{k + 1}"
        o[k] = rn[k]
        if k < 3:
            t1[k] = mr.conv2d(mr.relu(rn[k]), *p[name + ".resConfUnit1.conv1"])
            o[k] = path + (mr.conv2d(mr.relu(t1[k]), *p[name + ".resConfUnit1.conv2"]) + mr.relu(rn[k]))
        t2[k] = mr.conv2d(mr.relu(o[k]), *p[name + ".resConfUnit2.conv1"])
        path = mr.upsample2x(mr.conv2d(mr.relu(t2[k]), *p[name + ".resConfUnit2.conv2"]) + mr.relu(o[k]), True)
    h0 = mr.conv2d(path, *p["output_conv.0"])
    hup = mr.upsample2x(h0, False)
    t = mr.conv2d(hup, *p["output_conv.2"])
    s = mr.conv2d(mr.relu(t), *p["output_conv.4"])[:, 0]
    return {"rn": rn, "t1": t1, "o": o, "t2": t2, "p0": path, "h0": h0, "hup": hup, "t": t, "s": s}


def rectified(forward):
    """{name: tensor} of every tensor of decoder_forward that a ReLU reads (the masks of the backward)."""
    out = {"t": forward["t"], "s": forward["s"]}
    for k in range(4):
        out[f"o{k}"], out[f"t2_{k}"] = forward["o"][k], forward["t2"][k]
        if k < 3:
            out[f"rn{k}"], out[f"t1_{k}"] = forward["rn"][k], forward["t1"][k]
    return out


def decoder_grad_case(case):
    """{gw00 .. gw20, gb00 .. gb16, gm0 .. gm3} of a small decoder case, in the order of the decoder's weight and bias tables."""
    f, W, maps = decoder_forward(case), case["weights"], case["maps"]
    gw, gb, gm = [None] * 21, [None] * 17, [None] * 4
    head = head_grad_case({"gy": case["gy"], "x": f["hup"], "weight2": W[19], "bias2": case["biases"][15], "weight4": W[20],
                           "bias4": case["biases"][16], "non_negative": case["non_negative"]})
    gw[19], gb[15], gw[20], gb[16] = head["gw2"], head["gb2"], head["gw4"], head["gb4"]
    gh0 = upsample2x_grad(head["gx"], False)
    gw[18], gb[14] = conv_grad_weight(gh0, f["p0"], 3)
    gp = conv_grad_input(gh0, W[18])
    for k in range(4):
        w0 = 4 if k == 3 else 6 + 4 * (2 - k)
        u2 = w0 if k == 3 else w0 + 2
        g = upsample2x_grad(gp, True)
        go, gw[u2], gb[u2 - 4], gw[u2 + 1], gb[u2 - 3] = unit_backward(g, f["o"][k], f["t2"][k], W[u2:u2 + 2])
        gl = go
        if k < 3:
            gl, gw[w0], gb[w0 - 4], gw[w0 + 1], gb[w0 - 3] = unit_backward(go, f["rn"][k], f["t1"][k], W[w0:w0 + 2])
        gw[k], _ = conv_grad_weight(gl, maps[k], 3)
        gm[k] = conv_grad_input(gl, W[k])
        gp = go
    out = {f"gw{i:02d}": a for i, a in enumerate(gw)}
    out.update({f"gb{i:02d}": a for i, a in enumerate(gb)})
    out.update({f"gm{k}": a for k, a in enumerate(gm)})
    return out
