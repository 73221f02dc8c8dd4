"""float64 numpy restatement of torchvision's ResNet(Bottleneck, blocks, groups, width_per_group) in eval mode -- the backbone the
reference's MiDaS v2.1 builds (monodepth/midas_v2/blocks.py:6-31) -- for robust_cvd_amd/csrc/cvd_resnext.h, and the bar of the GPU
tests.  The mathematics in double, from the f32 inputs.  The fixture (resnext_golden.npz, minted by
tests/golden/reference_py/make_resnext_golden.py from STOCK TORCH f32 modules wired as torchvision's Bottleneck / ResNet; never from
the kernels) records how far torch's f32 arithmetic is from it.  The array functions need numpy only; the stock-torch modules import
torch when they are called."""
import os

import numpy as np

from tests import midas_reference as mr
from tests import raftenc_reference as er
from tests import resnext_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "resnext_golden.npz")
EPS32 = 2.0 ** -23
bar = er.bar


def conv2d(x, weight, stride=1):
    return er.conv2d(x, weight, np.zeros(weight.shape[0]), stride)


def grouped_conv2d(x, weight, stride, groups):
    x = np.asarray(x, np.float64)
    cg_in, cg_out = x.shape[1] // groups, weight.shape[0] // groups
    assert weight.shape[1] == cg_in and cg_in * groups == x.shape[1] and cg_out * groups == weight.shape[0]
    return np.concatenate([conv2d(x[:, g * cg_in:(g + 1) * cg_in], weight[g * cg_out:(g + 1) * cg_out], stride) for g in range(groups)],
                          axis=1)


def norm_relu(y, norm, relu=False, residual=None):
    """The kernels' epilogue: the eval batch norm, ReLU, max(residual + y, 0)."""
    if norm is not None:
        y = er.batch_norm(y, norm, rc.EPS)
    return er.epilogue(y, relu, residual)


def maxpool(x):
    """nn.MaxPool2d(3, 2, 1): padding counts as minus infinity."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    Ho, Wo = rc.out_size(H, 2), rc.out_size(W, 2)
    padded = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), constant_values=-np.inf)
    out = np.full(x.shape[:2] + (Ho, Wo), -np.inf)
    for i in range(3):
        for j in range(3):
            out = np.maximum(out, padded[:, :, i:i + 2 * (Ho - 1) + 1:2, j:j + 2 * (Wo - 1) + 1:2])
    return out


def grouped_case(case):
    return norm_relu(grouped_conv2d(case["x"], case["weight"], case["stride"], case["groups"]), case["norm"], case["relu"])


def conv_case(case):
    return norm_relu(conv2d(case["x"], case["weight"], case["stride"]), case["norm"], case["relu"], case["residual"])


def bottleneck(x, params, stride, groups):
    """params: [(weight, norm)] of conv1, conv2, conv3 (and downsample.0)."""
    x = np.asarray(x, np.float64)
    out = norm_relu(conv2d(x, params[0][0]), params[0][1], True)
    out = norm_relu(grouped_conv2d(out, params[1][0], stride, groups), params[1][1], True)
    identity = x if len(params) == 3 else norm_relu(conv2d(x, params[3][0], stride), params[3][1])
    return norm_relu(conv2d(out, params[2][0]), params[2][1], False, identity)


def block_case(case):
    return bottleneck(case["x"], case["params"], case["stride"], case["groups"])


def backbone(images, params, blocks, groups):
    """The four stages' outputs, f64; params in rc.conv_table's order."""
    x = maxpool(norm_relu(conv2d(images, params[0][0], 2), params[0][1], True))
    maps, at = [], 1
    for stage in range(4):
        for i in range(blocks[stage]):
            n = 4 if i == 0 else 3
            x = bottleneck(x, params[at:at + n], 2 if (stage > 0 and i == 0) else 1, groups)
            at += n
        maps.append(x)
    assert at == len(params)
    return maps


def backbone_case(case):
    return backbone(case["images"], case["params"], case["blocks"], case["groups"])


def net_case(case):
    return mr.decoder(backbone_case(case), case["decoder"], case["non_negative"])


def check_conditions(name, maps):
    """The conditions on a backbone case's feature maps: finite, between 10 % and 90 % zeros, a scale within [1e-3, 1e3]."""
    for k, m in enumerate(maps):
        zeros, scale = float((m == 0).mean()), float(np.abs(m).max())
        assert np.isfinite(m).all(), (name, k)
        assert 0.10 <= zeros <= 0.90, (name, k, zeros)
        assert 1e-3 <= scale <= 1e3, (name, k, scale)


# ---- the same network in stock torch ops (minting script, the live check and tools/midasnet_bench.py) ------------------------------
def stock_resnet(blocks, groups, width_per_group):
    """torchvision's ResNet(Bottleneck, blocks, groups=groups, width_per_group=width_per_group) up to layer4, written with
    nn.Conv2d(groups=...), nn.BatchNorm2d and nn.MaxPool2d under torchvision's member names (v1.5: the stride on conv2)."""
    import torch
    nn = torch.nn

    class Bottleneck(nn.Module):
        def __init__(self, inplanes, planes, stride, downsample):
            super().__init__()
            width = int(planes * (width_per_group / 64.0)) * groups
            self.conv1 = nn.Conv2d(inplanes, width, kernel_size=1, stride=1, bias=False)
            self.bn1 = nn.BatchNorm2d(width)
            self.conv2 = nn.Conv2d(width, width, kernel_size=3, stride=stride, padding=1, groups=groups, bias=False, dilation=1)
            self.bn2 = nn.BatchNorm2d(width)
            self.conv3 = nn.Conv2d(width, planes * 4, kernel_size=1, stride=1, bias=False)
            self.bn3 = nn.BatchNorm2d(planes * 4)
            self.relu = nn.ReLU(inplace=True)
            self.downsample = downsample

        def forward(self, x):
            identity = x
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.relu(self.bn2(self.conv2(out)))
            out = self.bn3(self.conv3(out))
            if self.downsample is not None:
                identity = self.downsample(x)
            out += identity
            return self.relu(out)

    class ResNet(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
            self.bn1 = nn.BatchNorm2d(64)
            self.relu = nn.ReLU(inplace=True)
            self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
            inplanes = 64
            for stage in range(4):
                planes, stride = 64 * 2 ** stage, 1 if stage == 0 else 2
                layers = []
                for i in range(blocks[stage]):
                    s = stride if i == 0 else 1
                    downsample = None
                    if s != 1 or inplanes != planes * 4:
                        downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, kernel_size=1, stride=s, bias=False), nn.BatchNorm2d(planes * 4))
                    layers.append(Bottleneck(inplanes, planes, s, downsample))
                    inplanes = planes * 4
                setattr(self, f"layer{stage + 1}", nn.Sequential(*layers))

    return ResNet()


def load_parameters(resnet, params, blocks, groups, width_per_group):
    """The case's parameters into a ResNet with torchvision's member names (strict)."""
    import torch
    sd = {}
    for (conv, norm, _k, _n, _shape, _s, _g, _last), (w, four) in zip(rc.conv_table(blocks, groups, width_per_group), params):
        sd[conv + ".weight"] = torch.from_numpy(w.copy())
        for v, a in zip(rc.NORM_KEYS, four):
            sd[f"{norm}.{v}"] = torch.from_numpy(a.copy())
        sd[f"{norm}.num_batches_tracked"] = torch.tensor(0)
    result = resnet.load_state_dict(sd, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    return resnet


def midas_backbone(resnet):
    """blocks.py:22-31 of the reference: the four stages of a ResNet as `pretrained.layer1 .. layer4`."""
    import torch
    pretrained = torch.nn.Module()
    pretrained.layer1 = torch.nn.Sequential(resnet.conv1, resnet.bn1, resnet.relu, resnet.maxpool, resnet.layer1)
    pretrained.layer2 = resnet.layer2
    pretrained.layer3 = resnet.layer3
    pretrained.layer4 = resnet.layer4
    return pretrained


def stock_backbone(case):
    """The case's backbone in stock torch ops with its parameters, as MidasNet.pretrained, in eval mode."""
    resnet = stock_resnet(case["blocks"], case["groups"], case["width_per_group"])
    load_parameters(resnet, case["params"], case["blocks"], case["groups"], case["width_per_group"])
    return midas_backbone(resnet).eval()


def stock_maps(pretrained, images):
    import torch
    with torch.no_grad():
        maps, x = [], torch.from_numpy(np.array(images)) if isinstance(images, np.ndarray) else images
        for k in range(4):
            x = getattr(pretrained, f"layer{k + 1}")(x)
            maps.append(x)
    return maps


def pretrained_state_dict(case):
    """The case's backbone parameters under the reference's `pretrained.*` names, as torch tensors, in the reference's order."""
    import torch
    sd = {}
    for (_c, _n, key, norm, _shape, _s, _g, _last), (w, four) in zip(
            rc.conv_table(case["blocks"], case["groups"], case["width_per_group"]), case["params"]):
        sd[f"pretrained.{key}.weight"] = torch.from_numpy(w.copy())
        for v, a in zip(rc.NORM_KEYS, four):
            sd[f"pretrained.{norm}.{v}"] = torch.from_numpy(a.copy())
        sd[f"pretrained.{norm}.num_batches_tracked"] = torch.tensor(0)
    return sd


def scratch_state_dict(case):
    return mr.scratch_state_dict({"params": case["decoder"]})


def reference_net(reference, case):
    """The reference's own MidasNet (midas_net.py) over the case's stock-torch backbone and the reference's own _make_scratch, with
    the case's parameters loaded (strict)."""
    blocks, midas_net = reference
    midas_net._make_encoder = lambda f, use_pretrained: (stock_backbone(case), blocks._make_scratch([256, 512, 1024, 2048], f))
    net = midas_net.MidasNet(path=None, features=case["features"], non_negative=case["non_negative"]).eval()
    sd = net.state_dict()
    sd.update(scratch_state_dict(case))
    net.load_state_dict(sd, strict=True)
    return net
