"""The decoder of robust_cvd_amd.midas with a backward, for fine-tuning:

    from robust_cvd_amd.midas_train import MidasNet
    net = MidasNet(path, backbone=midas.resnext101_32x8d(), freeze_backbone=True).cuda().train()
    loss = criterion(midas.estimate_depth(net, images)); loss.backward()

torch.autograd functions over the forward kernels of csrc/cvd_midas.h and the backward kernels of csrc/cvd_midas_grad.h
(cvd_midas_conv_grad_input_device, cvd_midas_conv_grad_weight_device, cvd_midas_upsample2x_grad_device, cvd_midas_head_grad_device),
each an enqueued library call on torch's current stream with no host synchronisation:

    conv2d(x, weight, bias, relu_in)        one stride-1 convolution; its input ReLU's mask is applied by the input gradient
    residual_unit(x, conv1, conv2, other)   conv2(relu(conv1(relu(x)))) + relu(x) (+ other): two launches forward; backward two weight
                                            gradients and two input gradients, the second with the skip path as its addend and x as mask
    upsample2x(x, align_corners)
    head(x, weight2, bias2, weight4, bias4, non_negative)

ResidualConvUnit, FeatureFusionBlock, Interpolate and MidasNet subclass the forward-only classes of robust_cvd_amd.midas, keep their
module names and state-dict keys, and accept training mode and tensors that require grad; the decoder has no batch norm and no
dropout, so .train() and .eval() compute the same function.  The forward values are those of the forward-only classes bit for bit
(the same launches).  A convolution with the epilogue ReLU flag has no differentiable path here; the decoder never uses it.

The backbone of MidasNet is a stock-torch module with layer1 .. layer4, run by torch under autograd (it receives the gradients of the
four feature maps); or a native midas.ResNeXt with freeze_backbone=True: its parameters do not require grad, it stays in eval mode
whatever .train() is called on the net, and it runs under no_grad, so the four layerK_rn input gradients -- the most expensive ones
-- are skipped; or a ResNeXt of THIS module (csrc/cvd_resnext_grad.h), which trains: batch-statistics norms in
training mode, every one of the 624-key parameters receives a gradient (midas_v21(path) builds that net, the reference's fine-tuning
form).  A forward-only midas.ResNeXt that is not frozen is refused: that class has no backward.

MidasNet.decode is ONE library call forward (cvd_midas_decoder_train_device, which writes the activations the backward needs into a
table of 16 tensors kept by autograd) and ONE backward (cvd_midas_decoder_backward_device); the block classes chain the operators.

Import this module (torch) before anything loads libcvd_hip.so.
"""
import ctypes as C

import torch

from . import api
from . import midas
from . import torch_common as tc
from .midas import NORM_MEAN, NORM_STDEV, estimate_depth  # noqa: F401  (the same function serves this class)

_i32 = C.c_int32


def _check(who, named):
    """CPU tensors, dtypes and devices; training mode and grad are accepted here."""
    for name, t in named.items():
        if not (torch.is_tensor(t) and t.is_cuda):
            raise ValueError(f"{who} runs on GPU tensors: {name} is not on a GPU (there is no CPU path)")
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: {name} must be float32 (got {t.dtype})")
    devices = {t.device for t in named.values()}
    if len(devices) != 1:
        raise ValueError(f"{who}: the tensors are on different devices ({sorted(map(str, devices))})")


def _plain(t):
    return None if t is None else t.detach().contiguous()


def _conv_forward(x, weight, bias, relu_in=False, a=None, relu_a=False, b=None):
    B, H, W, Cin, N, k = api.midas_check_conv(x.shape, weight.shape, None if bias is None else bias.shape,
                                              None if a is None else a.shape, None if b is None else b.shape)
    out = torch.empty((B, N, H, W), dtype=torch.float32, device=x.device)
    midas._call(x.device, "midas_conv_device", _i32(B), _i32(H), _i32(W), _i32(Cin), _i32(N), _i32(k), tc.ptr(x), tc.ptr(weight),
                tc.ptr(bias), _i32(1 if relu_in else 0), _i32(0), tc.ptr(a), _i32(1 if relu_a else 0), tc.ptr(b), _i32(0), tc.ptr(out))
    return out


def _grad_input(gy, weight, add=None, mask=None):
    B, H, W, Cin, N, k = api.midas_check_conv_grad_input(gy.shape, weight.shape, None if add is None else add.shape,
                                                         None if mask is None else mask.shape)
    gx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=gy.device)
    midas._call(gy.device, "midas_conv_grad_input_device", _i32(B), _i32(H), _i32(W), _i32(Cin), _i32(N), _i32(k), tc.ptr(gy), tc.ptr(weight),
                tc.ptr(add), tc.ptr(mask), _i32(0), tc.ptr(gx))
    return gx


def _grad_weight(gy, x, kernel_size, relu_in, with_bias):
    B, H, W, Cin, N, k = api.midas_check_conv_grad_weight(gy.shape, x.shape, kernel_size)
    gw = torch.empty((N, Cin, k, k), dtype=torch.float32, device=gy.device)
    gb = torch.empty((N,), dtype=torch.float32, device=gy.device) if with_bias else None
    midas._call(gy.device, "midas_conv_grad_weight_device", _i32(B), _i32(H), _i32(W), _i32(Cin), _i32(N), _i32(k), tc.ptr(gy), tc.ptr(x),
                _i32(1 if relu_in else 0), _i32(0), tc.ptr(gw), tc.ptr(gb))
    return gw, gb


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu_in):
        x, weight, bias = _plain(x), _plain(weight), _plain(bias)
        ctx.save_for_backward(x, weight)
        ctx.relu_in, ctx.with_bias = bool(relu_in), bias is not None
        return _conv_forward(x, weight, bias, relu_in=relu_in)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _grad_input(gy, weight, mask=x if ctx.relu_in else None)
        if ctx.needs_input_grad[1] or (ctx.with_bias and ctx.needs_input_grad[2]):
            gw, gb = _grad_weight(gy, x, weight.shape[2], ctx.relu_in, ctx.with_bias)
        return gx, gw, gb, None


class _ResidualUnit(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, other):
        x, w1, b1, w2, b2, other = (_plain(t) for t in (x, w1, b1, w2, b2, other))
        t1 = _conv_forward(x, w1, b1, relu_in=True)
        ctx.save_for_backward(x, t1, w1, w2)
        return _conv_forward(t1, w2, b2, relu_in=True, a=x, relu_a=True, b=other)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, t1, w1, w2 = ctx.saved_tensors
        gy = gy.contiguous()
        need = ctx.needs_input_grad
        gx = gw1 = gb1 = gw2 = gb2 = None
        if need[3] or need[4]:
            gw2, gb2 = _grad_weight(gy, t1, 3, True, True)
        if need[0] or need[1] or need[2]:
            g1 = _grad_input(gy, w2, mask=t1)                   # through conv2 and the ReLU in front of it
            if need[1] or need[2]:
                gw1, gb1 = _grad_weight(g1, x, 3, True, True)
            if need[0]:
                gx = _grad_input(g1, w1, add=gy, mask=x)        # (conv1's input gradient + the skip path) [x > 0]
        return gx, gw1, gb1, gw2, gb2, (gy if need[5] else None)


class _Upsample2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, align_corners):
        ctx.align = bool(align_corners)
        return midas._upsample2x(x, align_corners)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        gy = gy.contiguous()
        B, Cn, H, W = api.midas_check_upsample2x_grad(gy.shape)
        gx = torch.empty((B, Cn, H, W), dtype=torch.float32, device=gy.device)
        midas._call(gy.device, "midas_upsample2x_grad_device", _i32(B), _i32(Cn), _i32(H), _i32(W), _i32(1 if ctx.align else 0), tc.ptr(gy),
                    tc.ptr(gx))
        return gx, None


class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w2, b2, w4, b4, non_negative):
        tensors = [_plain(t) for t in (x, w2, b2, w4, b4)]
        B, H, W, Cin = api.midas_check_head(*[t.shape for t in tensors])
        ctx.save_for_backward(*tensors)
        ctx.non_negative, ctx.dims = bool(non_negative), (B, H, W, Cin)
        out = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
        midas._call(x.device, "midas_head_device", _i32(B), _i32(H), _i32(W), _i32(Cin), _i32(api.MIDAS_HEAD_MID), *[tc.ptr(t) for t in tensors],
                    _i32(1 if non_negative else 0), tc.ptr(out))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        tensors = ctx.saved_tensors
        B, H, W, Cin = ctx.dims
        gy = gy.contiguous()
        grads = [torch.empty_like(t) for t in tensors]
        midas._call(gy.device, "midas_head_grad_device", _i32(B), _i32(H), _i32(W), _i32(Cin), _i32(api.MIDAS_HEAD_MID), tc.ptr(gy),
                    *[tc.ptr(t) for t in tensors], _i32(1 if ctx.non_negative else 0), *[tc.ptr(g) for g in grads])
        return (*[g if n else None for g, n in zip(grads, ctx.needs_input_grad[:5])], None)


class _Decode(torch.autograd.Function):
    """The whole decoder: ONE library call forward (cvd_midas_decoder_train_device, which fills the saved-activation table) and ONE
    backward (cvd_midas_decoder_backward_device).  Arguments: the four feature maps, the 21 weights, the 17 biases."""

    @staticmethod
    def forward(ctx, non_negative, *tensors):
        tensors = [_plain(t) for t in tensors]
        maps, weights, biases = tensors[:4], tensors[4:25], tensors[25:]
        B, features, channels, heights, widths = api.midas_check_decoder([t.shape for t in maps], [t.shape for t in weights],
                                                                         [t.shape for t in biases])
        device = maps[0].device
        saved = [torch.empty(s, dtype=torch.float32, device=device) for s in api.midas_saved_shapes(B, features, heights, widths)]
        out = torch.empty((B, 4 * heights[0], 4 * widths[0]), dtype=torch.float32, device=device)
        ctx.dims = (B, features, channels, heights, widths)
        ctx.non_negative = bool(non_negative)
        midas._call(device, "midas_decoder_train_device", _i32(B), _i32(features), (_i32 * 4)(*channels), (_i32 * 4)(*heights),
                    (_i32 * 4)(*widths), _table(maps), _table(weights), _table(biases), _i32(1 if non_negative else 0), _table(saved),
                    tc.ptr(out))
        ctx.save_for_backward(*tensors, *saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        kept = ctx.saved_tensors
        maps, weights, biases, saved = kept[:4], kept[4:25], kept[25:42], kept[42:]
        B, features, channels, heights, widths = ctx.dims
        gy = gy.contiguous()
        gw, gb = [torch.empty_like(t) for t in weights], [torch.empty_like(t) for t in biases]
        gm = [torch.empty_like(t) for t in maps] if any(ctx.needs_input_grad[1:5]) else None
        midas._call(gy.device, "midas_decoder_backward_device", _i32(B), _i32(features), (_i32 * 4)(*channels), (_i32 * 4)(*heights),
                    (_i32 * 4)(*widths), tc.ptr(gy), _table(maps), _table(saved), _table(weights), _table(biases),
                    _i32(1 if ctx.non_negative else 0), _table(gw), _table(gb), None if gm is None else _table(gm))
        grads = (gm or [None] * 4) + gw + gb
        return (None, *[g if n else None for g, n in zip(grads, ctx.needs_input_grad[1:])])


def _table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def decode(maps, weights, biases, non_negative=True):
    """The decoder on the four feature maps with the 21 weights and 17 biases in api.MIDAS_PARAMETERS order -> [B, 4 H_1, 4 W_1]: one
    library call forward, one backward."""
    return _Decode.apply(bool(non_negative), *maps, *weights, *biases)


def conv2d(x, weight, bias=None, relu_in=False, relu=False):
    """One convolution of csrc/cvd_midas.h (stride 1, padding k // 2, k in (1, 3)) with a backward: conv(relu(x) under relu_in) +
    bias."""
    if relu:
        raise ValueError("conv2d: the epilogue ReLU has no differentiable path (the decoder never uses it)")
    _check("conv2d", {"x": x, "weight": weight, **({} if bias is None else {"bias": bias})})
    return _Conv2d.apply(x, weight, bias, bool(relu_in))


def residual_unit(x, conv1, conv2, other=None):
    """conv2(relu(conv1(relu(x)))) + relu(x) (+ other), conv1 and conv2 nn.Conv2d parameter holders."""
    return _ResidualUnit.apply(x, conv1.weight, conv1.bias, conv2.weight, conv2.bias, other)


def upsample2x(x, align_corners):
    _check("upsample2x", {"x": x})
    return _Upsample2x.apply(x, bool(align_corners))


def head(x, weight2, bias2, weight4, bias4, non_negative=True):
    """The output head in one launch (midas_net.py:38-41) with a backward."""
    _check("head", {"x": x, "weight2": weight2, "bias2": bias2, "weight4": weight4, "bias4": bias4})
    return _Head.apply(x, weight2, bias2, weight4, bias4, bool(non_negative))


class Interpolate(midas.Interpolate):
    def forward(self, x):
        return upsample2x(x, False)


class ResidualConvUnit(midas.ResidualConvUnit):
    def forward(self, x, other=None):
        named = {"x": x, **midas._parameters(self)}
        if other is not None:
            named["other"] = other
        _check("ResidualConvUnit", named)
        api.midas_check_conv(x.shape, self.conv1.weight.shape, self.conv1.bias.shape, None, None if other is None else other.shape)
        return residual_unit(x, self.conv1, self.conv2, other)


class FeatureFusionBlock(midas.FeatureFusionBlock):
    def __init__(self, features):
        torch.nn.Module.__init__(self)
        self.resConfUnit1 = ResidualConvUnit(features)
        self.resConfUnit2 = ResidualConvUnit(features)

    def forward(self, *xs):
        who = "FeatureFusionBlock"
        if len(xs) not in (1, 2):
            raise ValueError(f"{who}: one or two inputs are expected (got {len(xs)})")
        output = xs[0]
        if len(xs) == 2:
            if xs[0].shape != xs[1].shape:
                raise ValueError(f"{who}: the inputs must have one shape (got {tuple(xs[0].shape)}, {tuple(xs[1].shape)})")
            output = self.resConfUnit1(xs[1], other=xs[0])
        return upsample2x(self.resConfUnit2(output), True)


# ---- the backbone in training (csrc/cvd_resnext_grad.h) -------------------------------------------------------------
def _rx_bare_conv(x, weight, stride, groups):
    """The raw output of a backbone convolution: the forward kernels of csrc/cvd_resnext.h called with a null norm."""
    if groups > 1:
        B, H, W, G, cg, Ho, Wo = api.resnext_check_grouped_conv(x.shape, weight.shape, stride)
        out = torch.empty((B, G * cg, Ho, Wo), dtype=torch.float32, device=x.device)
        midas._call(x.device, "resnext_grouped_conv_device", _i32(B), _i32(H), _i32(W), _i32(G), _i32(cg), _i32(stride), tc.ptr(x),
                    tc.ptr(weight), None, C.c_float(api.RESNEXT_EPS), _i32(0), tc.ptr(out))
        return out
    B, H, W, Cin, N, k, Ho, Wo = api.resnext_check_conv(x.shape, weight.shape, stride)
    out = torch.empty((B, N, Ho, Wo), dtype=torch.float32, device=x.device)
    midas._call(x.device, "resnext_conv_device", _i32(B), _i32(H), _i32(W), _i32(Cin), _i32(N), _i32(k), _i32(stride), tc.ptr(x),
                tc.ptr(weight), None, C.c_float(api.RESNEXT_EPS), _i32(0), None, _i32(0), tc.ptr(out))
    return out


def _rx_norm(who, c, bn, relu, residual=None):
    """nn.BatchNorm2d `bn` on c in the mode of bn.training (each norm follows its own flag, as torch's) -> (y, mean, invstd); the
    running statistics and num_batches_tracked are updated in training mode."""
    midas._check_norm(who, bn)
    four = midas._norm_vectors(bn)
    B, N, H, W = api.resnext_check_norm_train(c.shape, [t.shape for t in four], bn.eps, bn.momentum, bn.training,
                                              None if residual is None else residual.shape)
    if not (bn.running_mean.is_contiguous() and bn.running_var.is_contiguous()):
        raise ValueError(f"{who}: the running statistics must be contiguous")
    gamma, beta = _plain(bn.weight), _plain(bn.bias)
    y = torch.empty_like(c)
    mean, invstd = (torch.empty((N,), dtype=torch.float32, device=c.device) for _ in range(2))
    midas._call(c.device, "resnext_norm_train_device", _i32(B), _i32(N), _i32(H), _i32(W), tc.ptr(c), tc.ptr(gamma), tc.ptr(beta),
                tc.ptr(bn.running_mean), tc.ptr(bn.running_var), C.c_double(bn.eps), C.c_double(bn.momentum),
                _i32(1 if bn.training else 0), _i32(1 if relu else 0), tc.ptr(residual), tc.ptr(mean), tc.ptr(invstd), tc.ptr(y))
    if bn.training:
        bn.num_batches_tracked.add_(1)
    return y, mean, invstd


def _rx_norm_grad(gy, c, y, mean, invstd, gamma, training, residual=False):
    B, N, H, W = api.resnext_check_norm_grad(gy.shape, c.shape, None if y is None else y.shape, [mean.shape, invstd.shape, gamma.shape],
                                             training)
    gc = torch.empty_like(c)
    gg, gb = (torch.empty((N,), dtype=torch.float32, device=c.device) for _ in range(2))
    gr = torch.empty_like(c) if residual else None
    midas._call(c.device, "resnext_norm_grad_device", _i32(B), _i32(N), _i32(H), _i32(W), tc.ptr(gy), tc.ptr(c), tc.ptr(y), tc.ptr(mean),
                tc.ptr(invstd), tc.ptr(gamma), _i32(1 if training else 0), tc.ptr(gc), tc.ptr(gg), tc.ptr(gb), tc.ptr(gr))
    return gc, gg, gb, gr


def _rx_conv_grad_weight(gy, x, weight, stride, groups):
    B, _, H, W = x.shape
    gw = torch.empty_like(weight)
    if groups > 1:
        _, _, _, G, cg = api.resnext_check_grouped_conv_grad_weight(gy.shape, x.shape, weight.shape[1], stride)
        midas._call(x.device, "resnext_grouped_conv_grad_weight_device", _i32(B), _i32(H), _i32(W), _i32(G), _i32(cg), _i32(stride),
                    tc.ptr(gy), tc.ptr(x), _i32(0), tc.ptr(gw))
        return gw
    _, _, _, Cin, N, k = api.resnext_check_conv_grad_weight(gy.shape, x.shape, weight.shape[2], stride)
    midas._call(x.device, "resnext_conv_grad_weight_device", _i32(B), _i32(H), _i32(W), _i32(Cin), _i32(N), _i32(k), _i32(stride),
                tc.ptr(gy), tc.ptr(x), _i32(0), tc.ptr(gw))
    return gw


class _BlockFn(torch.autograd.Function):
    """One Bottleneck: ONE library call forward (cvd_resnext_block_train_device, which fills the saved table: per convolution its
    raw output, mean, invstd and post-activation tensor -- the ReLU masks are the tensors the forward wrote) and ONE backward
    (cvd_resnext_block_backward_device).  Arguments: the module, x, then per convolution (conv1, conv2, conv3, downsample.0) its
    weight and its norm's weight and bias."""

    @staticmethod
    def forward(ctx, block, x, *params):
        x = _plain(x)
        params = [_plain(p) for p in params]
        bns = [block.bn1, block.bn2, block.bn3] + ([] if block.downsample is None else [block.downsample[1]])
        n = len(bns)
        for bn in bns:
            midas._check_norm("Bottleneck", bn)
            if bn.eps != bns[0].eps or bn.momentum != bns[0].momentum:
                raise ValueError("Bottleneck: the norms of a block must share eps and momentum")
            if not (bn.running_mean.is_contiguous() and bn.running_var.is_contiguous()):
                raise ValueError("Bottleneck: the running statistics must be contiguous")
        weights = params[0::3]
        norms = [[params[3 * i + 1], params[3 * i + 2], bn.running_mean, bn.running_var] for i, bn in enumerate(bns)]
        dims = api.resnext_check_block(x.shape, [w.shape for w in weights], [[t.shape for t in four] for four in norms],
                                       block.conv2.stride[0], bns[0].eps, bns[0].momentum, [bn.training for bn in bns])
        B, H, W, Cin, width, out, G, stride, down, flags = dims
        saved = [torch.empty(sh, dtype=torch.float32, device=x.device)
                 for sh in api.resnext_block_saved_shapes(B, H, W, Cin, width, out, stride, down)]
        ctx.dims = dims
        ctx.scalars = [_i32(v) for v in (B, H, W, Cin, width, out, G, stride, int(down))]
        midas._call(x.device, "resnext_block_train_device", *ctx.scalars, tc.ptr(x), _table(weights),
                    _table([t for four in norms for t in four]), C.c_double(bns[0].eps), C.c_double(bns[0].momentum),
                    (_i32 * n)(*[int(f) for f in flags]), _table(saved))
        for bn in bns:
            if bn.training:
                bn.num_batches_tracked.add_(1)
        ctx.save_for_backward(x, *params, *saved)
        return saved[11]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        flags = ctx.dims[9]
        n = len(flags)
        kept = ctx.saved_tensors
        x, params, saved = kept[0], kept[1:1 + 3 * n], kept[1 + 3 * n:]
        gy = gy.contiguous()
        weights, gammas = params[0::3], params[1::3]
        gx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        gw, gg, gb = ([torch.empty_like(t) for t in group] for group in (weights, gammas, gammas))
        midas._call(x.device, "resnext_block_backward_device", *ctx.scalars, tc.ptr(gy), tc.ptr(x), _table(weights), _table(gammas),
                    _table(saved), (_i32 * n)(*[int(f) for f in flags]), tc.ptr(gx), _table(gw), _table(gg), _table(gb))
        grads = [t for three in zip(gw, gg, gb) for t in three]
        return (None, gx, *[g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:])])


class _StemFn(torch.autograd.Function):
    """conv1 7 x 7 / 2, bn1, ReLU, the pool; the images receive no gradient (that kernel is not built)."""

    @staticmethod
    def forward(ctx, stem, x, weight, gamma, beta):
        x, weight, gamma = _plain(x), _plain(weight), _plain(gamma)
        c = _rx_bare_conv(x, weight, 2, 1)
        y, mean, invstd = _rx_norm("ResNeXt.layer1.1", c, stem[1], True)
        ctx.training = stem[1].training
        ctx.save_for_backward(x, weight, gamma, c, y, mean, invstd)
        return midas._rx_maxpool(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gp):
        x, weight, gamma, c, y, mean, invstd = ctx.saved_tensors
        gp = gp.contiguous()
        B, Cn, H, W = api.resnext_check_maxpool_grad(y.shape, gp.shape)
        gyv = torch.empty_like(y)
        midas._call(y.device, "resnext_maxpool_grad_device", _i32(B), _i32(Cn), _i32(H), _i32(W), tc.ptr(y), tc.ptr(gp), tc.ptr(gyv))
        gc, gg, gb, _ = _rx_norm_grad(gyv, c, y, mean, invstd, gamma, ctx.training)
        gw = _rx_conv_grad_weight(gc, x, weight, 2, 1)
        return None, None, gw, gg, gb


class Bottleneck(midas.Bottleneck):
    """midas.Bottleneck with a backward: the same members and state-dict keys.  Each norm follows its own .training flag: batch
    statistics (the running ones and num_batches_tracked updated) or the running statistics."""

    def forward(self, x):
        _check("Bottleneck", {"x": x, **midas._tensors(self)})
        convs = [(self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)]
        if self.downsample is not None:
            convs.append((self.downsample[0], self.downsample[1]))
        return _BlockFn.apply(self, x, *[t for conv, bn in convs for t in (conv.weight, bn.weight, bn.bias)])


class _Stem(midas._Stem):
    def forward(self, x):
        _check("ResNeXt.layer1", {"x": x, **midas._tensors(self)})
        if torch.is_grad_enabled() and x.requires_grad:
            raise ValueError("ResNeXt.layer1: the images require grad, and the stem's input gradient has no kernel")
        return self[4](_StemFn.apply(self, x, self[0].weight, self[1].weight, self[1].bias))


class ResNeXt(midas.ResNeXt):
    """midas.ResNeXt with a backward: the same modules and the reference checkpoint's 624 `pretrained.*` keys.
    layer1 .. layer4 run their stages under autograd, a torch.autograd.Function per block; .train() runs the norms on batch
    statistics as the reference's fine-tuning does, .eval() with parameters that require grad is the frozen-statistics form.  In
    eval mode with grad mode off, forward(x) is midas.ResNeXt's one-call inference path."""

    def __init__(self, blocks=api.RESNEXT101_32X8D[0], groups=api.RESNEXT101_32X8D[1], width_per_group=api.RESNEXT101_32X8D[2]):
        super().__init__(blocks, groups, width_per_group)
        # (the parent's constructor builds its own forward-only blocks: the same members, so the class alone changes.  Both
        # classes are module-level and importable, which copy.deepcopy and pickling of the net rely on.)
        for m in self.modules():
            if type(m) is midas.Bottleneck:
                m.__class__ = Bottleneck
            elif type(m) is midas._Stem:
                m.__class__ = _Stem

    def forward(self, x):
        who = "ResNeXt"
        if not torch.is_grad_enabled() and not any(m.training for m in self.modules()):
            return super().forward(x)
        _check(who, {"x": x})
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"{who}: x must be (B, 3, H, W) (got {tuple(x.shape)})")
        if x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError(f"{who}: height and width must be multiples of 32 (got {x.shape[2]} x {x.shape[3]})")
        maps = []
        for k in (1, 2, 3, 4):
            maps.append(getattr(self, f"layer{k}")(maps[-1] if maps else x))
        return maps


def resnext101_32x8d():
    """The architecture of the reference's `resnext101_32x8d_wsl` backbone with a backward, with no weights: nothing is fetched."""
    return ResNeXt(*api.RESNEXT101_32X8D)


def midas_v21(path=None, freeze_backbone=False):
    """The reference's MidasNet(path) (midas_net.py:13-29) as depth_fine_tuning.py trains it: the native backbone and decoder, every
    parameter trainable unless freeze_backbone."""
    return MidasNet(path, backbone=resnext101_32x8d(), freeze_backbone=freeze_backbone)


class MidasNet(midas.MidasNet):
    """midas.MidasNet with a differentiable decoder: the same modules, names and 42 `scratch.*` state-dict keys, so the reference's
    checkpoint and its `save` round-trip.  freeze_backbone: see the module's text."""

    def __init__(self, path=None, features=256, non_negative=True, backbone=None, backbone_channels=api.MIDAS_BACKBONE_CHANNELS,
                 freeze_backbone=False):
        torch.nn.Module.__init__(self)       # (midas.MidasNet's constructor with this module's blocks: nothing is allocated twice)
        features = int(features)
        if features < 1:
            raise ValueError(f"MidasNet: features must be >= 1 (got {features})")
        self.pretrained = midas._make_resnext101_32x8d() if backbone is None else backbone
        for k in (1, 2, 3, 4):
            if not hasattr(self.pretrained, f"layer{k}"):
                raise ValueError(f"MidasNet: the backbone has no layer{k}")
        self.scratch = midas._make_scratch(list(backbone_channels), features)
        for k in (4, 3, 2, 1):
            setattr(self.scratch, f"refinenet{k}", FeatureFusionBlock(features))
        self.scratch.output_conv = torch.nn.Sequential(
            torch.nn.Conv2d(features, 128, kernel_size=3, stride=1, padding=1),
            Interpolate(scale_factor=2, mode="bilinear"),
            torch.nn.Conv2d(128, api.MIDAS_HEAD_MID, kernel_size=3, stride=1, padding=1),
            torch.nn.ReLU(True),
            torch.nn.Conv2d(api.MIDAS_HEAD_MID, 1, kernel_size=1, stride=1, padding=0),
            torch.nn.ReLU(True) if non_negative else torch.nn.Identity(),
        )
        self.non_negative = bool(non_negative)
        self.freeze_backbone = bool(freeze_backbone)
        native = isinstance(self.pretrained, midas.ResNeXt)
        if native and not isinstance(self.pretrained, ResNeXt) and not self.freeze_backbone:
            raise ValueError("MidasNet: training the forward-only midas.ResNeXt backbone has no kernel yet (that class has no "
                             "backward): pass a midas_train.ResNeXt, freeze_backbone=True, or a stock-torch backbone")
        if self.freeze_backbone:
            for p in self.pretrained.parameters():
                p.requires_grad_(False)
            self.pretrained.eval()
        if path:
            self.load(path)

    def train(self, mode=True):
        super().train(mode)
        if self.freeze_backbone:
            self.pretrained.eval()
        return self

    def decode(self, layer_1, layer_2, layer_3, layer_4):
        who = "MidasNet"
        maps = [layer_1, layer_2, layer_3, layer_4]
        s = self.scratch
        convs = [s.get_submodule(n) for n in api.MIDAS_PARAMETERS]
        named = {**{f"layer_{k + 1}": t for k, t in enumerate(maps)},
                 **{f"scratch.{n}.weight": m.weight for n, m in zip(api.MIDAS_PARAMETERS, convs)},
                 **{f"scratch.{n}.bias": m.bias for n, m in zip(api.MIDAS_PARAMETERS[4:], convs[4:])}}
        _check(who, named)
        api.midas_check_decoder([t.shape for t in maps], [m.weight.shape for m in convs], [m.bias.shape for m in convs[4:]])
        return decode(maps, [m.weight for m in convs], [m.bias for m in convs[4:]], self.non_negative)

    def forward(self, x):
        who = "MidasNet"
        _check(who, {"x": x})
        if x.dim() != 4:
            raise ValueError(f"{who}: x must be (B, C, H, W) (got {tuple(x.shape)})")
        if x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError(f"{who}: height and width must be multiples of 32 (got {x.shape[2]} x {x.shape[3]})")
        if any(p.device != x.device for p in self.parameters()):
            raise ValueError(f"{who}: the parameters and the images are on different devices")
        if self.freeze_backbone:
            with torch.no_grad():
                if isinstance(self.pretrained, midas.ResNeXt):
                    maps = self.pretrained(x)
                else:
                    maps = []
                    for k in (1, 2, 3, 4):
                        maps.append(getattr(self.pretrained, f"layer{k}")(maps[-1] if maps else x))
            return self.decode(*maps)
        layer_1 = self.pretrained.layer1(x)
        layer_2 = self.pretrained.layer2(layer_1)
        layer_3 = self.pretrained.layer3(layer_2)
        layer_4 = self.pretrained.layer4(layer_3)
        return self.decode(layer_1, layer_2, layer_3, layer_4)
