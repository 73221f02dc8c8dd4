"""float64 numpy restatement of the reference's MiDaS v2.1 decoder (monodepth/midas_v2/blocks.py:41-159 Interpolate,
ResidualConvUnit, FeatureFusionBlock; midas_net.py:57-74 MidasNet.forward behind the backbone) for robust_cvd_amd/csrc/cvd_midas.h,
and the bar of the GPU tests.  The mathematics in double, from the f32 inputs.  The fixture (midas_golden.npz, minted by
tests/golden/reference_py/make_midas_golden.py from the reference's OWN classes) records how far the reference's f32 arithmetic is
from it.  The array functions need numpy only; load_reference and the stock-torch decoder import torch when they are called.

ResidualConvUnit: the reference's nn.ReLU(inplace=True) rectifies the caller's tensor before `out + x`, so the unit computes
conv2(relu(conv1(relu(x)))) + relu(x).  residual_conv_unit(inplace=False) is the form the source text seems to say, kept so that
tests/test_midas_reference.py can show the fixture tells the two apart."""
import os
import sys
import types

import numpy as np

from tests import midas_cases as mc
from tests import raftenc_reference as er

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "midas_golden.npz")
EPS32 = 2.0 ** -23
bar = er.bar


def relu(x):
    return np.maximum(np.asarray(x, np.float64), 0.0)


def conv2d(x, weight, bias=None):
    y = er.conv2d(x, weight, np.zeros(weight.shape[0]) if bias is None else bias, 1)
    return y


def conv_case(case):
    """The kernel's contract: t = conv(relu_in ? relu(x) : x) + bias; relu; t + (relu_a ? relu(a) : a); b + t."""
    x = relu(case["x"]) if case["relu_in"] else case["x"]
    t = conv2d(x, case["weight"], case["bias"])
    if case["relu"]:
        t = relu(t)
    if case["a"] is not None:
        t = t + (relu(case["a"]) if case["relu_a"] else np.asarray(case["a"], np.float64))
    if case["b"] is not None:
        t = np.asarray(case["b"], np.float64) + t
    return t


def upsample2x(x, align_corners):
    """torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=...) in f64."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]

    def axis(n):
        d = np.arange(2 * n, dtype=np.float64)
        if align_corners:
            src = d * ((n - 1) / (2 * n - 1)) if 2 * n > 1 else 0.0 * d
        else:
            src = np.maximum((d + 0.5) * 0.5 - 0.5, 0.0)
        i0 = np.minimum(src.astype(np.int64), n - 1)
        i1 = np.minimum(i0 + 1, n - 1)
        l1 = src - i0
        return i0, i1, 1.0 - l1, l1
    y0, y1, h0, h1 = axis(H)
    x0, x1, w0, w1 = axis(W)
    rows = x[..., y0, :] * h0[:, None] + x[..., y1, :] * h1[:, None]
    return rows[..., x0] * w0 + rows[..., x1] * w1


def residual_conv_unit(x, weights, biases, inplace=True):
    r = relu(x)
    out = conv2d(relu(conv2d(r, weights[0], biases[0])), weights[1], biases[1])
    return out + (r if inplace else np.asarray(x, np.float64))


def feature_fusion_block(xs, weights, biases, inplace=True):
    """weights / biases: resConfUnit1.conv1, .conv2, resConfUnit2.conv1, .conv2."""
    out = np.asarray(xs[0], np.float64)
    if len(xs) == 2:
        out = out + residual_conv_unit(xs[1], weights[0:2], biases[0:2], inplace)
    out = residual_conv_unit(out, weights[2:4], biases[2:4], inplace)
    return upsample2x(out, True)


def head(x, weight2, bias2, weight4, bias4, non_negative):
    y = conv2d(relu(conv2d(x, weight2, bias2)), weight4, bias4)[:, 0]
    return relu(y) if non_negative else y


def decoder(maps, params, non_negative=True, inplace=True):
    """MidasNet.forward from the four feature maps; params {layer name: (weight, bias)} -> [B, 4 H_1, 4 W_1] f64."""
    def p(prefix):
        names = [f"{prefix}.resConfUnit{u}.conv{c}" for u in (1, 2) for c in (1, 2)]
        return [params[n][0] for n in names], [params[n][1] for n in names]
    rn = [conv2d(m, params[f"layer{k + 1}_rn"][0]) for k, m in enumerate(maps)]
    path = feature_fusion_block([rn[3]], *p("refinenet4"), inplace)
    for k in (3, 2, 1):
        path = feature_fusion_block([path, rn[k - 1]], *p(f"refinenet{k}"), inplace)
    y = upsample2x(conv2d(path, *params["output_conv.0"]), False)
    return head(y, *params["output_conv.2"], *params["output_conv.4"], non_negative)


def unit_case(case, inplace=True):
    return residual_conv_unit(case["x"], case["weights"], case["biases"], inplace)


def fusion_case(case, inplace=True):
    return feature_fusion_block([case["x0"], case["x1"]], case["weights"], case["biases"], inplace)


def head_case(case):
    return head(case["x"], case["weight2"], case["bias2"], case["weight4"], case["bias4"], case["non_negative"])


def decoder_case(case):
    return decoder(case["maps"], case["params"], case["non_negative"])


# ---- the reference's classes (minting script and the live check, CPU only) --------------------------------------------------------
def load_reference():
    """(blocks, midas_net) modules of the reference checkout (ROBUST_CVD_REFERENCE, default /root/reference), or None where it (or
    torch) is not available.  blocks.py imports iopath and torchvision at module level and neither is needed by the decoder: stub
    modules stand in for exactly those names while it is imported.  torch.hub.load is replaced by a function that raises for the
    life of the process: nothing here may fetch."""
    root = os.environ.get("ROBUST_CVD_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(root, "monodepth", "midas_v2", "blocks.py")):
        return None
    try:
        import torch
    except ImportError:
        return None

    def refuse(*a, **k):
        raise RuntimeError("torch.hub.load must not run: nothing here may fetch")
    torch.hub.load = refuse
    stubs = {}
    for name, attrs in (("iopath", {}), ("iopath.common", {}), ("iopath.common.file_io", {"PathManager": type("PathManager", (), {})}),
                        ("torchvision", {}), ("torchvision.models", {}),
                        ("torchvision.models.resnet", {"ResNet": type("ResNet", (), {}), "Bottleneck": type("Bottleneck", (), {})})):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            stubs[name] = m
    sys.modules.update(stubs)
    added = root not in sys.path
    if added:
        sys.path.insert(0, root)
    try:
        from monodepth.midas_v2 import blocks, midas_net
    finally:
        if added:
            sys.path.remove(root)
        for name in stubs:
            sys.modules.pop(name, None)
    return blocks, midas_net


def stub_backbone(stub):
    """The stub backbone of a decoder case as a torch module with layer1 .. layer4 (tests/midas_cases.py: STUB_LAYERS)."""
    import torch
    backbone = torch.nn.Module()
    for i, ((cin, cout, k), entry) in enumerate(zip(mc.STUB_LAYERS, stub)):
        conv = torch.nn.Conv2d(cin, cout, kernel_size=k, stride=k, bias=False)
        conv.weight.data.copy_(torch.from_numpy(mc.stub_weight(i, entry)))
        setattr(backbone, f"layer{i + 1}", conv)
    return backbone


def reference_net(reference, case):
    """The reference's MidasNet over the case's stub backbone, with the case's parameters loaded (strict)."""
    import torch
    blocks, midas_net = reference
    features = case["features"]
    midas_net._make_encoder = lambda f, use_pretrained: (stub_backbone(case["stub"]), blocks._make_scratch(list(mc.BACKBONE_CHANNELS), f))
    net = midas_net.MidasNet(path=None, features=features, non_negative=case["non_negative"]).eval()
    sd = net.state_dict()
    sd.update(scratch_state_dict(case))
    net.load_state_dict(sd, strict=True)
    return net


def scratch_state_dict(case):
    """The decoder case's parameters under the reference's 42 `scratch.*` names, as torch tensors."""
    import torch
    sd = {}
    for name in mc.STATE_DICT_LAYERS:
        w, b = case["params"][name]
        sd[f"scratch.{name}.weight"] = torch.from_numpy(w.copy())
        if b is not None:
            sd[f"scratch.{name}.bias"] = torch.from_numpy(b.copy())
    return {k: sd[k] for k in mc.STATE_DICT_KEYS}
