"""float64 numpy restatement of the reference's encoder (raft/core/extractor.py:8-60 ResidualBlock, :124-197 BasicEncoder in eval
mode) for robust_cvd_amd/csrc/cvd_raftenc.h, and the bar of the GPU tests.  The mathematics in double, from the f32 inputs: the
convolution as im2col + matmul, the eval batch norm from its four vectors, the instance norm with the biased variance.  The fixture
(raftenc_golden.npz, minted by tests/golden/reference_py/make_raftenc_golden.py) records how far the reference's own f32 arithmetic
is from it.  The array functions need numpy only; stock_raft (the whole network in stock torch ops, for the torch child and the
minting script) imports torch when it is called."""
import os
import sys

import numpy as np

from tests import raftenc_cases as ec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "raftenc_golden.npz")
EPS32 = 2.0 ** -23


def conv2d(x, weight, bias, stride=1):
    """x [B, C, H, W]; weight [O, C, k, k], zero padding k // 2 -> conv + bias, [B, O, ceil(H / stride), ceil(W / stride)] f64."""
    x = np.asarray(x, np.float64)
    weight = np.asarray(weight, np.float64)
    B, C, H, W = x.shape
    O, C2, k, k2 = weight.shape
    assert C == C2 and k == k2 and k % 2 == 1
    r = k // 2
    Ho, Wo = (H + 2 * r - k) // stride + 1, (W + 2 * r - k) // stride + 1
    padded = np.pad(x, ((0, 0), (0, 0), (r, r), (r, r)))
    columns = np.empty((B, C, k, k, Ho, Wo), np.float64)
    for i in range(k):
        for j in range(k):
            columns[:, :, i, j] = padded[:, :, i:i + stride * (Ho - 1) + 1:stride, j:j + stride * (Wo - 1) + 1:stride]
    out = np.matmul(weight.reshape(O, C * k * k), columns.reshape(B, C * k * k, Ho * Wo)).reshape(B, O, Ho, Wo)
    return out + np.asarray(bias, np.float64).reshape(1, O, 1, 1)


def batch_norm(y, four, eps=ec.EPS):
    gamma, beta, mean, var = (np.asarray(a, np.float64).reshape(1, -1, 1, 1) for a in four)
    return (y - mean) / np.sqrt(var + eps) * gamma + beta


def instance_norm(y, eps=ec.EPS):
    y = np.asarray(y, np.float64)
    if y.shape[2] * y.shape[3] < 2:
        raise ValueError("Expected more than 1 spatial element")
    mean = y.mean(axis=(2, 3), keepdims=True)
    var = ((y - mean) ** 2).mean(axis=(2, 3), keepdims=True)
    return (y - mean) / np.sqrt(var + eps)


def epilogue(y, relu, residual):
    if relu:
        y = np.maximum(y, 0.0)
    if residual is not None:
        y = np.maximum(np.asarray(residual, np.float64) + y, 0.0)
    return y


def conv_case(case):
    y = conv2d(case["x"], case["weight"], case["bias"], case["stride"])
    if case["norm"] is not None:
        y = batch_norm(y, case["norm"])
    return epilogue(y, case["relu"], case["residual"])


def norm_case(case):
    return epilogue(instance_norm(case["x"]), case["relu"], case["residual"])


def encoder(images, weights, biases, norm_mode, norms=None, eps=ec.EPS):
    """BasicEncoder.forward in eval mode -> [B, output_dim, ceil(H / 8), ceil(W / 8)] f64."""
    def layer(i, x, relu, residual=None):
        y = conv2d(x, weights[i], biases[i], ec.LAYERS[i][4])
        if i < 15 and norm_mode == "batch":
            y = batch_norm(y, norms[i], eps)
        elif i < 15 and norm_mode == "instance":
            y = instance_norm(y, eps)
        return epilogue(y, relu, residual)

    def block(i, x, strided):
        y = layer(i, x, True)
        if strided:
            x = layer(i + 2, x, False)
        return layer(i + 1, y, True, x)
    x = layer(0, images, True)
    x = block(3, block(1, x, False), False)
    x = block(8, block(5, x, True), False)
    x = block(13, block(10, x, True), False)
    return layer(15, x, False)


def encoder_case(case):
    return encoder(case["images"], case["weights"], case["biases"], case["norm_mode"], case["norms"])


def bar(delta, scale):
    """The project's f32 bar against the f64 restatement: 8 x the reference's own f32 error for the case (never below one f32 ulp
    of the output scale)."""
    return 8.0 * max(float(delta), EPS32 * float(scale))


# ---- the reference's modules (minting script, CPU only) and the network in stock torch ops ----------------------------------------
def load_reference():
    """(BasicEncoder, RAFT) of the reference checkout (ROBUST_CVD_REFERENCE, default /root/reference), or None where it (or torch)
    is not available."""
    root = os.environ.get("ROBUST_CVD_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(root, "raft", "core", "extractor.py")):
        return None
    try:
        import torch  # noqa: F401
    except ImportError:
        return None
    added = root not in sys.path
    if added:
        sys.path.insert(0, root)
    try:
        from raft.core.extractor import BasicEncoder
        from raft.core.raft import RAFT
    finally:
        if added:
            sys.path.remove(root)
    return BasicEncoder, RAFT


def encoder_state_dict(case, norm_mode=None):
    """The encoder case's parameters under the reference's names, as torch tensors."""
    import torch
    norm_mode = norm_mode or case["norm_mode"]
    sd = {}
    for n, w, b in zip(ec.PARAMETERS, case["weights"], case["biases"]):
        sd[n + ".weight"], sd[n + ".bias"] = torch.from_numpy(w.copy()), torch.from_numpy(b.copy())
    if norm_mode == "batch":
        for n, four in zip(ec.NORMS, case["norms"]):
            for m in [n] + ([n.replace("norm3", "downsample.1")] if n.endswith("norm3") else []):
                for v, a in zip(ec.NORM_VECTORS, four):
                    sd[f"{m}.{v}"] = torch.from_numpy(a.copy())
                sd[f"{m}.num_batches_tracked"] = torch.tensor(7)
    return {k: sd[k] for k in ec.encoder_keys("", norm_mode)}


def raft_state_dict(case):
    import torch
    return {k: torch.from_numpy(np.array(v)) for k, v in case["state"].items()}


def stock_encoder(sd, prefix, norm_mode, x):
    """BasicEncoder.forward in eval mode with stock torch functions, at x's dtype, from a state dict."""
    import torch.nn.functional as F

    def layer(name, norm, x, stride, relu, residual=None):
        w = sd[f"{prefix}{name}.weight"].to(x.dtype)
        y = F.conv2d(x, w, sd[f"{prefix}{name}.bias"].to(x.dtype), stride=stride, padding=w.shape[2] // 2)
        if norm is not None and norm_mode == "batch":
            g, b, m, v = (sd[f"{prefix}{norm}.{n}"].to(x.dtype) for n in ec.NORM_VECTORS)
            y = F.batch_norm(y, m, v, g, b, training=False, eps=ec.EPS)
        elif norm is not None and norm_mode == "instance":
            y = F.instance_norm(y, eps=ec.EPS)
        if relu:
            y = F.relu(y)
        return y if residual is None else F.relu(residual + y)

    x = layer("conv1", "norm1", x, 2, True)
    for l, strided in ((1, False), (2, True), (3, True)):
        for blk in (0, 1):
            b = f"layer{l}.{blk}."
            s = 2 if strided and blk == 0 else 1
            y = layer(b + "conv1", b + "norm1", x, s, True)
            if s == 2:
                x = layer(b + "downsample.0", b + "norm3", x, 2, False)
            x = layer(b + "conv2", b + "norm2", y, 1, True, x)
    return layer("conv2", None, x, 1, False)


def stock_raft(sd, image1, image2, iters, dtype, flow_init=None):
    """raft/core/raft.py:62-116 (test_mode) restated with stock torch ops on the CPU at `dtype` (the reference's own modules cannot
    run in f64: its corr.py casts to float): -> (flow at 1/8, upsampled flow)."""
    import torch
    from tests.raftblock_torch_child import StockBlock, stock_lookup, stock_upsample
    with torch.no_grad():
        image1 = 2 * (image1.to(dtype) / 255.0) - 1.0
        image2 = 2 * (image2.to(dtype) / 255.0) - 1.0
        fmap1 = stock_encoder(sd, "fnet.", "instance", image1)
        fmap2 = stock_encoder(sd, "fnet.", "instance", image2)
        net, inp = torch.split(stock_encoder(sd, "cnet.", "batch", image1), [128, 128], dim=1)
        net, inp = torch.tanh(net), torch.relu(inp)
        block = StockBlock()
        block.load_state_dict({k[len("update_block."):]: v for k, v in sd.items() if k.startswith("update_block.")})
        block = block.to(dtype)
        B, dim, h, w = fmap1.shape
        corr = torch.matmul(fmap1.view(B, dim, h * w).transpose(1, 2), fmap2.view(B, dim, h * w)).view(B * h * w, 1, h, w) / dim ** 0.5
        pyramid = [corr]
        for _ in range(3):
            pyramid.append(torch.nn.functional.avg_pool2d(pyramid[-1], 2, stride=2))
        ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
        coords0 = torch.stack([xs, ys], 0)[None].repeat(B, 1, 1, 1)
        coords1 = coords0.clone() if flow_init is None else coords0 + flow_init.to(dtype)
        for _ in range(iters):
            net, mask, delta = block(net, inp, stock_lookup(pyramid, coords1, 4), coords1 - coords0)
            coords1 = coords1 + delta
        return coords1 - coords0, stock_upsample(coords1 - coords0, mask)
