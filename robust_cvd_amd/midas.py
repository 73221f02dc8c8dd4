"""Drop-in for the reference's MiDaS v2.1 depth network (monodepth/midas_v2/midas_net.py, blocks.py) on GPU tensors:

    from robust_cvd_amd.midas import midas_v21, estimate_depth
    net = midas_v21("models/midas_v21-f6b98070.pt").cuda().eval()     # MidasNet(path, backbone=resnext101_32x8d())
    depth = estimate_depth(net, images)                               # MidasV2Model.estimate_depth

The kernels are csrc/cvd_midas.h (the decoder) and csrc/cvd_resnext.h (the backbone, §3.20).  MidasNet has the
reference's module names and its 42 `scratch.*` state-dict keys in its order; with backbone=resnext101_32x8d() also the 624
`pretrained.*` keys of the ResNeXt-101 32x8d in the reference's order, so the reference's checkpoint loads with strict=True.  The
backbone (`pretrained`) is either a ResNeXt of this module -- ONE call of the library (cvd_midas_backbone_device) for the four
feature maps -- or any stock-torch module with layer1 .. layer4; everything behind it -- the four layerK_rn convolutions, the
four FeatureFusionBlocks and the output head -- is ONE call of the library (cvd_midas_decoder_device).  Both run on torch's
current stream with no host synchronisation.
ResidualConvUnit, FeatureFusionBlock and Interpolate are the reference's blocks on the same kernels, one library call per launch.

The reference's ResidualConvUnit holds an nn.ReLU(inplace=True): it rectifies the caller's tensor before `out + x`, so it computes
conv2(relu(conv1(relu(x)))) + relu(x).  The modules here compute that and leave the caller's tensors as they are.

Forward only, float32, eval mode.  Raised before any device work: a CPU tensor, a dtype other than float32, a module in training
mode, an input or parameter that requires grad while grad mode is on, tensors on more than one device (ValueError / TypeError /
RuntimeError), and the shape errors of the operators (ValueError): image sides must be multiples of 32.  Nothing here fetches: with
backbone=None the ResNeXt-101 32x8d is built locally from torchvision's classes, an ImportError where torchvision is missing.

Import this module (torch) before anything loads libcvd_hip.so.
"""
import ctypes as C

import torch

from . import api
from . import torch_common as tc

NORM_MEAN = (0.485, 0.456, 0.406)
NORM_STDEV = (0.229, 0.224, 0.225)


def _check(who, module, named):
    """The refusals every forward shares: training mode, CPU tensors, dtypes, grad, devices."""
    if module is not None and module.training:
        raise ValueError(f"{who}: training mode has no kernel (forward only): call .eval()")
    for name, t in named.items():
        if not (torch.is_tensor(t) and t.is_cuda):
            raise ValueError(f"{who} runs on GPU tensors: {name} is not on a GPU (there is no CPU path)")
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: {name} must be float32 (got {t.dtype})")
        if torch.is_grad_enabled() and t.requires_grad:
            raise RuntimeError(f"{who} is forward only: {name} requires grad (call it under torch.no_grad())")
    devices = {t.device for t in named.values()}
    if len(devices) != 1:
        raise ValueError(f"{who}: the tensors are on different devices ({sorted(map(str, devices))})")


def _call(device, name, *args):
    handle = tc.solver(device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        handle._check(handle._fn(name)(handle._h, *args, C.c_void_p(stream)))


def _conv(x, conv, relu_in=False, a=None, relu_a=False, b=None):
    """One launch (two with a split K) of csrc/cvd_midas.h: conv(relu(x) under relu_in) + bias, + relu(a) under relu_a, + b."""
    bias = conv.bias
    B, H, W, Cin, N, k = api.midas_check_conv(x.shape, conv.weight.shape, None if bias is None else bias.shape,
                                              None if a is None else a.shape, None if b is None else b.shape)
    x, weight = x.detach().contiguous(), conv.weight.detach().contiguous()
    bias, a, b = (None if t is None else t.detach().contiguous() for t in (bias, a, b))
    out = torch.empty((B, N, H, W), dtype=torch.float32, device=x.device)
    _call(x.device, "midas_conv_device", C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(Cin), C.c_int32(N), C.c_int32(k), tc.ptr(x),
          tc.ptr(weight), tc.ptr(bias), C.c_int32(1 if relu_in else 0), C.c_int32(0), tc.ptr(a), C.c_int32(1 if relu_a else 0), tc.ptr(b),
          C.c_int32(0), tc.ptr(out))
    return out


def _upsample2x(x, align_corners):
    B, Cn, H, W = api.midas_check_upsample2x(x.shape)
    x = x.detach().contiguous()
    out = torch.empty((B, Cn, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    _call(x.device, "midas_upsample2x_device", C.c_int32(B), C.c_int32(Cn), C.c_int32(H), C.c_int32(W), C.c_int32(1 if align_corners else 0),
          tc.ptr(x), tc.ptr(out))
    return out


def _parameters(module):
    return {n: p for n, p in module.named_parameters()}


class Interpolate(torch.nn.Module):
    """The reference's Interpolate (blocks.py:41-74) for what MidasNet uses it for: scale_factor 2, bilinear, align_corners=False."""

    def __init__(self, scale_factor, mode):
        super().__init__()
        if scale_factor != 2 or mode != "bilinear":
            raise ValueError(f"Interpolate: scale_factor 2 and mode 'bilinear' are the only kernel (got {scale_factor}, {mode!r})")
        self.scale_factor = scale_factor
        self.mode = mode

    def forward(self, x):
        _check("Interpolate", None, {"x": x})
        return _upsample2x(x, False)


class ResidualConvUnit(torch.nn.Module):
    """The reference's ResidualConvUnit (blocks.py:77-117) with its parameter names: conv2(relu(conv1(relu(x)))) + relu(x) -- the
    in-place ReLU of the reference makes the skip relu(x).  Two launches; x is not modified."""

    def __init__(self, features):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(features, features, kernel_size=3, stride=1, padding=1, bias=True)
        self.conv2 = torch.nn.Conv2d(features, features, kernel_size=3, stride=1, padding=1, bias=True)
        self.relu = torch.nn.ReLU(inplace=True)        # (the reference's member; never called)

    def forward(self, x, other=None):
        """`other` (FeatureFusionBlock): added to the result in the second launch's epilogue."""
        who = "ResidualConvUnit"
        named = {"x": x, **_parameters(self)}
        if other is not None:
            named["other"] = other
        _check(who, self, named)
        return _conv(_conv(x, self.conv1, relu_in=True), self.conv2, relu_in=True, a=x, relu_a=True, b=other)


class FeatureFusionBlock(torch.nn.Module):
    """The reference's FeatureFusionBlock (blocks.py:120-159) with its module names: xs[0] (+ resConfUnit1(xs[1])), resConfUnit2,
    bilinear x 2 with align_corners=True.  Four convolution launches and the upsampling; the inputs are not modified."""

    def __init__(self, features):
        super().__init__()
        self.resConfUnit1 = ResidualConvUnit(features)
        self.resConfUnit2 = ResidualConvUnit(features)

    def forward(self, *xs):
        who = "FeatureFusionBlock"
        if len(xs) not in (1, 2):
            raise ValueError(f"{who}: one or two inputs are expected (got {len(xs)})")
        _check(who, self, {**{f"xs[{i}]": t for i, t in enumerate(xs)}, **_parameters(self)})
        output = xs[0]
        if len(xs) == 2:
            if xs[0].shape != xs[1].shape:
                raise ValueError(f"{who}: the inputs must have one shape (got {tuple(xs[0].shape)}, {tuple(xs[1].shape)})")
            output = self.resConfUnit1(xs[1], other=xs[0])
        return _upsample2x(self.resConfUnit2(output), True)


def _norm_vectors(bn):
    return [bn.weight, bn.bias, bn.running_mean, bn.running_var]


def _check_norm(who, bn):
    if not isinstance(bn, torch.nn.BatchNorm2d) or not bn.affine or not bn.track_running_stats:
        raise ValueError(f"{who}: the norm must be an affine nn.BatchNorm2d with running statistics")


def _rx_conv(x, conv, bn, relu, residual=None):
    """One launch (two with a split K) of csrc/cvd_resnext.h's dense convolution: bn(conv(x)), ReLU, max(residual + y, 0)."""
    norm = [t.detach().contiguous() for t in _norm_vectors(bn)]
    B, H, W, Cin, N, k, Ho, Wo = api.resnext_check_conv(x.shape, conv.weight.shape, tuple(conv.stride), [t.shape for t in norm], bn.eps,
                                                        None if residual is None else residual.shape)
    x, weight = x.detach().contiguous(), conv.weight.detach().contiguous()
    residual = None if residual is None else residual.detach().contiguous()
    out = torch.empty((B, N, Ho, Wo), dtype=torch.float32, device=x.device)
    _call(x.device, "resnext_conv_device", C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(Cin), C.c_int32(N), C.c_int32(k),
          C.c_int32(conv.stride[0]), tc.ptr(x), tc.ptr(weight), (C.c_void_p * 4)(*[t.data_ptr() for t in norm]), C.c_float(bn.eps),
          C.c_int32(1 if relu else 0), tc.ptr(residual), C.c_int32(0), tc.ptr(out))
    return out


def _rx_grouped_conv(x, conv, bn, relu):
    norm = [t.detach().contiguous() for t in _norm_vectors(bn)]
    B, H, W, G, cg, Ho, Wo = api.resnext_check_grouped_conv(x.shape, conv.weight.shape, tuple(conv.stride), [t.shape for t in norm], bn.eps)
    x, weight = x.detach().contiguous(), conv.weight.detach().contiguous()
    out = torch.empty((B, G * cg, Ho, Wo), dtype=torch.float32, device=x.device)
    _call(x.device, "resnext_grouped_conv_device", C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(G), C.c_int32(cg),
          C.c_int32(conv.stride[0]), tc.ptr(x), tc.ptr(weight), (C.c_void_p * 4)(*[t.data_ptr() for t in norm]), C.c_float(bn.eps),
          C.c_int32(1 if relu else 0), tc.ptr(out))
    return out


def _rx_maxpool(x):
    B, Cn, H, W, Ho, Wo = api.resnext_check_maxpool(x.shape)
    x = x.detach().contiguous()
    out = torch.empty((B, Cn, Ho, Wo), dtype=torch.float32, device=x.device)
    _call(x.device, "resnext_maxpool_device", C.c_int32(B), C.c_int32(Cn), C.c_int32(H), C.c_int32(W), tc.ptr(x), tc.ptr(out))
    return out


def _tensors(module):
    """parameters and the norms' running statistics (not num_batches_tracked, which no kernel reads)"""
    named = {n: p for n, p in module.named_parameters()}
    named.update({n: b for n, b in module.named_buffers() if not n.endswith("num_batches_tracked")})
    return named


class Bottleneck(torch.nn.Module):
    """torchvision's Bottleneck (v1.5: the stride sits on the grouped 3 x 3) with its member names, as parameter holder; forward runs
    csrc/cvd_resnext.h: conv1 + bn1 + ReLU, conv2 + bn2 + ReLU, the downsample branch where there is one, conv3 + bn3 + the
    residual + ReLU -- three or four launches (and the folds of split convolutions).  x is not modified."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64):
        super().__init__()
        width = int(planes * (base_width / 64.0)) * groups
        self.conv1 = torch.nn.Conv2d(inplanes, width, kernel_size=1, stride=1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(width)
        self.conv2 = torch.nn.Conv2d(width, width, kernel_size=3, stride=stride, padding=1, groups=groups, bias=False)
        self.bn2 = torch.nn.BatchNorm2d(width)
        self.conv3 = torch.nn.Conv2d(width, planes * self.expansion, kernel_size=1, stride=1, bias=False)
        self.bn3 = torch.nn.BatchNorm2d(planes * self.expansion)
        self.relu = torch.nn.ReLU(inplace=True)        # (torchvision's member; never called)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        who = "Bottleneck"
        _check(who, self, {"x": x, **_tensors(self)})
        out = _rx_conv(x, self.conv1, self.bn1, True)
        out = _rx_grouped_conv(out, self.conv2, self.bn2, True)
        identity = x if self.downsample is None else _rx_conv(x, self.downsample[0], self.downsample[1], False)
        return _rx_conv(out, self.conv3, self.bn3, False, residual=identity)


class _Stem(torch.nn.Sequential):
    """`pretrained.layer1` of the reference (blocks.py:22-31): Sequential(conv1, bn1, relu, maxpool, layer1) with its indices as
    state-dict names; forward runs the stem convolution with its norm and ReLU in one launch, the pool, then the blocks."""

    def forward(self, x):
        _check("ResNeXt.layer1", self, {"x": x, **_tensors(self)})
        x = _rx_maxpool(_rx_conv(x, self[0], self[1], True))
        return self[4](x)


class ResNeXt(torch.nn.Module):
    """torchvision's ResNet(Bottleneck, blocks, groups=groups, width_per_group=width_per_group) behind the reference's
    _make_resnet_backbone: layer1 = Sequential(conv1, bn1, relu, maxpool, layer1), layer2 .. layer4 the stages, so that as
    MidasNet.pretrained it has the reference checkpoint's keys in its order (api.resnext_state_dict_keys).  The modules are plain
    nn.Conv2d / nn.BatchNorm2d as parameter holders.  layer1 .. layer4 are callable: each runs its stage on the kernels, a launch per
    convolution; forward(x) returns the four feature maps from ONE library call (cvd_midas_backbone_device)."""

    def __init__(self, blocks=api.RESNEXT101_32X8D[0], groups=api.RESNEXT101_32X8D[1], width_per_group=api.RESNEXT101_32X8D[2]):
        super().__init__()
        self.blocks = tuple(int(b) for b in blocks)
        self.groups, self.width_per_group = int(groups), int(width_per_group)
        self._table = api.resnext_conv_table(self.blocks, self.groups, self.width_per_group)
        inplanes = 64
        stages = []
        for k, count in enumerate(self.blocks):
            planes, stride = 64 << k, 1 if k == 0 else 2
            layers = []
            for i in range(count):
                downsample = None
                if i == 0:
                    downsample = torch.nn.Sequential(
                        torch.nn.Conv2d(inplanes, planes * Bottleneck.expansion, kernel_size=1, stride=stride, bias=False),
                        torch.nn.BatchNorm2d(planes * Bottleneck.expansion))
                layers.append(Bottleneck(inplanes, planes, stride if i == 0 else 1, downsample, self.groups, self.width_per_group))
                inplanes = planes * Bottleneck.expansion
            stages.append(torch.nn.Sequential(*layers))
        self.layer1 = _Stem(torch.nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False), torch.nn.BatchNorm2d(64),
                            torch.nn.ReLU(inplace=True), torch.nn.MaxPool2d(kernel_size=3, stride=2, padding=1), stages[0])
        self.layer2, self.layer3, self.layer4 = stages[1:]
        self._tables = None         # (device, tensors kept alive, weight pointers, norm pointers): rebuilt when the module moves

    @property
    def out_channels(self):
        return tuple(256 << k for k in range(4))

    def _apply(self, fn, *args, **kwargs):
        self._tables = None
        return super()._apply(fn, *args, **kwargs)

    def _pointer_tables(self, who, x):
        """The weight and norm tables of cvd_midas_backbone_device in api.resnext_conv_table's order, checked once per placement."""
        if self._tables is not None and self._tables[0] == x.device and all(t.data_ptr() == p for t, p in self._tables[4]):
            return self._tables
        named, weights, norms = {}, [], []
        for c in self._table:
            conv, bn = self.get_submodule(c.key), self.get_submodule(c.norm_key)
            _check_norm(who, bn)
            if bn.eps != api.RESNEXT_EPS:
                raise ValueError(f"{who}: {c.norm_key}.eps must be {api.RESNEXT_EPS} (got {bn.eps})")
            named[c.key + ".weight"] = conv.weight
            weights.append(conv.weight)
            four = _norm_vectors(bn)
            named.update({f"{c.norm_key}.{v}": t for v, t in zip(api.RESNEXT_NORM_VECTORS, four)})
            norms.append(four)
        _check(who, None, {"x": x, **named})
        api.resnext_check_backbone(x.shape, self.blocks, self.groups, self.width_per_group, [t.shape for t in weights],
                                   [[t.shape for t in four] for four in norms])
        keep = [t.detach().contiguous() for t in weights] + [t.detach().contiguous() for four in norms for t in four]
        n = len(weights)
        # (the first and the last tensor's addresses stand for the placement: parameters swapped one by one need a new module)
        sentinels = [(weights[0], weights[0].data_ptr()), (norms[-1][3], norms[-1][3].data_ptr())]
        self._tables = (x.device, keep, (C.c_void_p * n)(*[t.data_ptr() for t in keep[:n]]),
                        (C.c_void_p * (4 * n))(*[t.data_ptr() for t in keep[n:]]), sentinels)
        return self._tables

    def forward(self, x):
        who = "ResNeXt"
        _check(who, self, {"x": x})
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"{who}: x must be (B, 3, H, W) (got {tuple(x.shape)})")
        if x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError(f"{who}: height and width must be multiples of 32 (got {x.shape[2]} x {x.shape[3]})")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError(f"{who} is forward only: its parameters require grad (call it under torch.no_grad())")
        _device, _keep, weights, norms, _s = self._pointer_tables(who, x)
        B, _, H, W = x.shape
        x = x.detach().contiguous()
        outs = [torch.empty((B, 256 << k, H >> (k + 2), W >> (k + 2)), dtype=torch.float32, device=x.device) for k in range(4)]
        _call(x.device, "midas_backbone_device", C.c_int32(B), C.c_int32(H), C.c_int32(W), (C.c_int32 * 4)(*self.blocks),
              C.c_int32(self.groups), C.c_int32(self.width_per_group), C.c_float(api.RESNEXT_EPS), tc.ptr(x), weights, norms,
              (C.c_void_p * 4)(*[t.data_ptr() for t in outs]))
        return outs


def resnext101_32x8d():
    """The architecture of the reference's `resnext101_32x8d_wsl` backbone on this module's kernels, with no weights: nothing is
    fetched (the checkpoint of MidasNet holds the backbone's weights)."""
    return ResNeXt(*api.RESNEXT101_32X8D)


def midas_v21(path=None):
    """The reference's MidasNet(path) (midas_net.py:13-29) with the native backbone: features 256, non-negative output."""
    return MidasNet(path, backbone=resnext101_32x8d())


def _make_resnet_backbone(resnet):
    """blocks.py:22-31: the four stages of a torchvision ResNet as `pretrained.layer1 .. layer4`."""
    pretrained = torch.nn.Module()
    pretrained.layer1 = torch.nn.Sequential(resnet.conv1, resnet.bn1, resnet.relu, resnet.maxpool, resnet.layer1)
    pretrained.layer2 = resnet.layer2
    pretrained.layer3 = resnet.layer3
    pretrained.layer4 = resnet.layer4
    return pretrained


def _make_resnext101_32x8d():
    """The architecture of the reference's `resnext101_32x8d_wsl` backbone, from torchvision's own classes, with no weights:
    nothing is fetched (the checkpoint of MidasNet holds the backbone's weights)."""
    try:
        from torchvision.models.resnet import Bottleneck, ResNet
    except ImportError as e:
        raise ImportError("MidasNet(backbone=None) builds the ResNeXt-101 32x8d backbone from torchvision, which is not installed; "
                          "install torchvision or pass backbone= a module with layer1 .. layer4") from e
    return _make_resnet_backbone(ResNet(Bottleneck, [3, 4, 23, 3], groups=32, width_per_group=8))


def _make_scratch(in_shape, out_shape):
    scratch = torch.nn.Module()
    for k, cin in enumerate(in_shape):
        setattr(scratch, f"layer{k + 1}_rn", torch.nn.Conv2d(cin, out_shape, kernel_size=3, stride=1, padding=1, bias=False))
    return scratch


class MidasNet(torch.nn.Module):
    """The reference's MidasNet (midas_net.py:13-74) with its module names: `pretrained` (the backbone) and `scratch` (the decoder:
    42 state-dict keys in the reference's order).  forward(x), x [B, 3, H, W] normalised images with H and W multiples of 32,
    returns the inverse depth [B, H, W]: the backbone's four feature maps -- ONE library call where `pretrained` is a ResNeXt of
    this module (cvd_midas_backbone_device), else its four stages as the modules they are --, then ONE library call
    for the whole decoder (cvd_midas_decoder_device, §3.19).  backbone: a module with layer1 .. layer4 whose outputs halve from stage
    to stage (channel counts are read from the feature maps' convolutions: `backbone_channels`); None builds the ResNeXt-101 32x8d
    from torchvision.  path: a checkpoint to load (strict=False, as the reference's BaseModel.load).  The scratch is the device
    handle's: calls on one device are ordered on one stream."""

    def __init__(self, path=None, features=256, non_negative=True, backbone=None, backbone_channels=api.MIDAS_BACKBONE_CHANNELS):
        super().__init__()
        features = int(features)
        if features < 1:
            raise ValueError(f"MidasNet: features must be >= 1 (got {features})")
        self.pretrained = _make_resnext101_32x8d() if backbone is None else backbone
        for k in (1, 2, 3, 4):
            if not hasattr(self.pretrained, f"layer{k}"):
                raise ValueError(f"MidasNet: the backbone has no layer{k}")
        self.scratch = _make_scratch(list(backbone_channels), features)
        self.scratch.refinenet4 = FeatureFusionBlock(features)
        self.scratch.refinenet3 = FeatureFusionBlock(features)
        self.scratch.refinenet2 = FeatureFusionBlock(features)
        self.scratch.refinenet1 = FeatureFusionBlock(features)
        # (modules for the reference's names, shapes and default initialisation; the Sequential's forward is never called)
        self.scratch.output_conv = torch.nn.Sequential(
            torch.nn.Conv2d(features, 128, kernel_size=3, stride=1, padding=1),
            Interpolate(scale_factor=2, mode="bilinear"),
            torch.nn.Conv2d(128, api.MIDAS_HEAD_MID, kernel_size=3, stride=1, padding=1),
            torch.nn.ReLU(True),
            torch.nn.Conv2d(api.MIDAS_HEAD_MID, 1, kernel_size=1, stride=1, padding=0),
            torch.nn.ReLU(True) if non_negative else torch.nn.Identity(),
        )
        self.non_negative = bool(non_negative)
        if path:
            self.load(path)

    def load(self, path):
        """base_model.py:6-17."""
        parameters = torch.load(path, map_location="cpu")
        if "optimizer" in parameters:
            parameters = parameters["model"]
        self.load_state_dict(parameters, strict=False)

    def decode(self, layer_1, layer_2, layer_3, layer_4):
        """The decoder on the backbone's four feature maps -> [B, 4 H_1, 4 W_1]."""
        who = "MidasNet"
        maps = [layer_1, layer_2, layer_3, layer_4]
        convs = [self.scratch.get_submodule(n) for n in api.MIDAS_PARAMETERS]
        weights = [m.weight for m in convs]
        biases = [m.bias for m in convs[4:]]
        named = {**{f"layer_{k + 1}": t for k, t in enumerate(maps)},
                 **{f"scratch.{n}.weight": w for n, w in zip(api.MIDAS_PARAMETERS, weights)},
                 **{f"scratch.{n}.bias": b for n, b in zip(api.MIDAS_PARAMETERS[4:], biases)}}
        _check(who, self, named)
        B, features, channels, heights, widths = api.midas_check_decoder([t.shape for t in maps], [t.shape for t in weights],
                                                                         [t.shape for t in biases])
        maps = [t.detach().contiguous() for t in maps]
        weights = [t.detach().contiguous() for t in weights]
        biases = [t.detach().contiguous() for t in biases]
        out = torch.empty((B, 4 * heights[0], 4 * widths[0]), dtype=torch.float32, device=maps[0].device)
        _call(out.device, "midas_decoder_device", C.c_int32(B), C.c_int32(features), (C.c_int32 * 4)(*channels), (C.c_int32 * 4)(*heights),
              (C.c_int32 * 4)(*widths), (C.c_void_p * 4)(*[t.data_ptr() for t in maps]), (C.c_void_p * 21)(*[t.data_ptr() for t in weights]),
              (C.c_void_p * 17)(*[t.data_ptr() for t in biases]), C.c_int32(1 if self.non_negative else 0), tc.ptr(out))
        return out

    def forward(self, x):
        who = "MidasNet"
        _check(who, self, {"x": x})
        if x.dim() != 4:
            raise ValueError(f"{who}: x must be (B, C, H, W) (got {tuple(x.shape)})")
        if x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError(f"{who}: height and width must be multiples of 32 (got {x.shape[2]} x {x.shape[3]})")
        if any(p.device != x.device for p in self.parameters()):
            raise ValueError(f"{who}: the parameters and the images are on different devices")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError(f"{who} is forward only: its parameters require grad (call it under torch.no_grad())")
        if isinstance(self.pretrained, ResNeXt):
            return self.decode(*self.pretrained(x))
        layer_1 = self.pretrained.layer1(x)
        layer_2 = self.pretrained.layer2(layer_1)
        layer_3 = self.pretrained.layer3(layer_2)
        layer_4 = self.pretrained.layer4(layer_3)
        return self.decode(layer_1, layer_2, layer_3, layer_4)


def estimate_depth(net, images):
    """MidasV2Model.estimate_depth (monodepth/midas_v2_model.py:44-62): images [..., C, H, W] in 0..1 -> depth [..., H, W] =
    1 / (1e-7 + net((images - mean) / stdev)).  The elementwise parts are torch ops on the images' device."""
    shape = images.shape
    Cn, H, W = shape[-3:]
    input_ = images.reshape(-1, Cn, H, W)
    mean = torch.tensor(NORM_MEAN, dtype=input_.dtype, device=input_.device).reshape(1, -1, 1, 1)
    stdev = torch.tensor(NORM_STDEV, dtype=input_.dtype, device=input_.device).reshape(1, -1, 1, 1)
    input_ = (input_ - mean) / stdev
    output = net(input_)
    disparity = output.reshape(shape[:-3] + output.shape[-2:])
    epsilon = 0.0000001
    return (epsilon + disparity).reciprocal()
