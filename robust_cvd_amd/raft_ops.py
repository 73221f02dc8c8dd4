"""Drop-ins for the two stages of the reference's RAFT (raft/core) that are neither a convolution nor a matmul, on GPU tensors:

    from robust_cvd_amd.raft_ops import CorrBlock, upsample_flow
    corr_fn = CorrBlock(fmap1, fmap2, num_levels=4, radius=4)     # raft/core/corr.py:8-23: matmul (torch's), then ONE launch
    corr = corr_fn(coords1)                                       # raft/core/corr.py:25-46: ONE launch per call
    flow_up = upsample_flow(flow, mask)                           # raft/core/raft.py:49-60: ONE launch

The kernels are csrc/cvd_raftops.h; INTEGRATION.md has the two edits to raft/core/raft.py.  Forward only, float32
only: RAFT computes flow under torch.no_grad().  Every call is enqueued on torch's current stream with no host synchronisation and
no scratch of the library's; the tensors are torch's.  CorrBlock keeps `corr_pyramid` as the reference does, a list of
[B h1 w1, 1, h, w] tensors, and the reference's output layout, [B, L (2 r + 1)^2, h1, w1] with the FIRST window index moving x.

Raised before any device work: a CPU tensor, a dtype other than float32, an input that requires grad while grad mode is on
(ValueError / TypeError / RuntimeError), and the domain errors of the operators (ValueError): 1..4 levels, radius 1..4, a coarsest
level below 2 x 2 (NaN in the reference).

SepConvGRU is the recurrent core of the update block (raft/core/update.py:37-75) with the reference's parameter names, on
csrc/cvd_raftgru.h: `from robust_cvd_amd.raft_ops import SepConvGRU` in raft/core/update.py.  It refuses, with
ValueError / TypeError and before any device work, other sizes than (128, 256), segments of x that are not multiples of 32
channels, CPU tensors, other dtypes, and an input or parameter that requires grad while grad mode is on.

BasicMotionEncoder, FlowHead and BasicUpdateBlock are the rest of the update block (raft/core/update.py:8-16, 96-114, 133-156)
with the reference's parameter names, on csrc/cvd_raftconv.h: `from robust_cvd_amd.raft_ops import
BasicUpdateBlock` in raft/core/update.py (or raft/core/raft.py).  A block call is 8 launches beside the GRU's 4, no cat, on the
current stream; the same domain rules and error types as SepConvGRU.

ResidualBlock, BasicEncoder and RAFT are the encoders and the whole network (raft/core/extractor.py:8-60, 124-197,
raft/core/raft.py) with the reference's module, parameter and buffer names, on csrc/cvd_raftenc.h:
`from robust_cvd_amd.raft_ops import RAFT` where optical_flow_homography.py imports the class is the whole integration; the
reference's checkpoint loads with strict=True.  An encoder call is one library call of 16 convolution launches (plus two per instance
norm); eval mode only.  SmallEncoder, BottleneckBlock and SmallUpdateBlock (args.small) are out of scope and refused.

Import this module (torch) before anything loads libcvd_hip.so.
"""
import ctypes as C

import torch

from . import api
from . import torch_common as tc


def _check(who, **tensors):
    for name, t in tensors.items():
        if not (torch.is_tensor(t) and t.is_cuda):
            raise ValueError(f"{who} runs on GPU tensors: {name} is not on a GPU (there is no CPU path)")
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: {name} must be float32 (got {t.dtype})")
        if torch.is_grad_enabled() and t.requires_grad:
            raise RuntimeError(f"{who} is forward only: {name} requires grad (call it under torch.no_grad())")
    devices = {t.device for t in tensors.values()}
    if len(devices) != 1:
        raise ValueError(f"{who}: the tensors are on different devices ({sorted(map(str, devices))})")


def _call(device, name, *args):
    handle = tc.solver(device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        handle._check(handle._fn(name)(handle._h, *args, C.c_void_p(stream)))


class CorrBlock:
    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        _check("CorrBlock", fmap1=fmap1, fmap2=fmap2)
        if fmap1.dim() != 4 or fmap1.shape != fmap2.shape:
            raise ValueError(f"CorrBlock: fmap1 and fmap2 must be (B, dim, h, w) alike (got {tuple(fmap1.shape)}, {tuple(fmap2.shape)})")
        self.num_levels = int(num_levels)
        self.radius = api.raft_check_radius(radius)
        batch, dim, ht, wd = fmap1.shape
        shapes = api.raft_level_shapes(ht, wd, self.num_levels)
        api.raft_check_dim(dim)
        self._shape = (batch, ht, wd)
        with torch.no_grad():
            raw = torch.matmul(fmap1.reshape(batch, dim, ht * wd).transpose(1, 2), fmap2.reshape(batch, dim, ht * wd))
            Q = batch * ht * wd
            levels = [raw.view(Q, 1, ht, wd)] + [torch.empty((Q, 1, h, w), dtype=torch.float32, device=raw.device)
                                                 for h, w in shapes[1:]]
            self._table = (C.c_void_p * len(levels))(*[t.data_ptr() for t in levels])
            # (level 0 is the product itself, scaled in place)
            _call(raw.device, "raft_corr_pyramid_device", C.c_int64(Q), C.c_int32(ht), C.c_int32(wd), C.c_int32(dim),
                  C.c_int32(len(levels)), tc.ptr(raw), self._table)
        self.corr_pyramid = levels

    def __call__(self, coords):
        _check("CorrBlock", coords=coords)
        batch, ht, wd = self._shape
        if tuple(coords.shape) != (batch, 2, ht, wd):
            raise ValueError(f"CorrBlock: coords must be {(batch, 2, ht, wd)} (got {tuple(coords.shape)})")
        if coords.device != self.corr_pyramid[0].device:
            raise ValueError(f"CorrBlock: coords is on {coords.device}, the pyramid on {self.corr_pyramid[0].device}")
        coords = coords.detach().contiguous()
        n = 2 * self.radius + 1
        out = torch.empty((batch, self.num_levels * n * n, ht, wd), dtype=torch.float32, device=coords.device)
        _call(coords.device, "raft_corr_lookup_device", C.c_int32(batch), C.c_int32(ht), C.c_int32(wd), C.c_int32(ht), C.c_int32(wd),
              C.c_int32(self.num_levels), C.c_int32(self.radius), self._table, tc.ptr(coords), tc.ptr(out))
        return out


class SepConvGRU(torch.nn.Module):
    """The reference's SepConvGRU(hidden_dim=128, input_dim=256) (raft/core/update.py:37-75) with its parameter names and shapes,
    so the update block's part of a RAFT state dict loads unchanged; forward(h, x) is four launches of csrc/cvd_raftgru.h
    (DESIGN.md §3.16).  x is one [B, 256, H, W] tensor or a tuple of up to three whose channel counts are multiples of 32 and sum
    to 256: the tuple is read where its tensors lie, no cat is formed.  Forward only, float32, GPU tensors; the result is a new
    tensor.  The scratch is the device handle's: calls on one device are ordered on one stream."""

    def __init__(self, hidden_dim=128, input_dim=256):
        super().__init__()
        if (hidden_dim, input_dim) != (api.GRU_HIDDEN, api.GRU_INPUT):
            raise ValueError(f"SepConvGRU: hidden_dim = {api.GRU_HIDDEN} and input_dim = {api.GRU_INPUT} are the only sizes of the "
                             f"kernel (BasicUpdateBlock's); got {hidden_dim}, {input_dim}")
        for name in api.GRU_PARAMETERS:
            kernel = api.raft_gru_weight_shape(name)[2:]
            # (a Conv2d for the parameter names, shapes and default initialisation of the reference; its forward is never called)
            setattr(self, name, torch.nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel, padding=(kernel[0] // 2, kernel[1] // 2)))

    def forward(self, h, x):
        who = "SepConvGRU"
        segs = tuple(x) if isinstance(x, (tuple, list)) else (x,)
        weights = [getattr(self, n).weight for n in api.GRU_PARAMETERS]
        biases = [getattr(self, n).bias for n in api.GRU_PARAMETERS]
        named = {"h": h, **{f"x[{i}]": t for i, t in enumerate(segs)},
                 **{f"{n}.weight": w for n, w in zip(api.GRU_PARAMETERS, weights)},
                 **{f"{n}.bias": b for n, b in zip(api.GRU_PARAMETERS, biases)}}
        for name, t in named.items():
            if not (torch.is_tensor(t) and t.is_cuda):
                raise ValueError(f"{who} runs on GPU tensors: {name} is not on a GPU (there is no CPU path)")
            if t.dtype != torch.float32:
                raise TypeError(f"{who}: {name} must be float32 (got {t.dtype})")
            if torch.is_grad_enabled() and t.requires_grad:
                raise ValueError(f"{who} is forward only: {name} requires grad (call it under torch.no_grad())")
        if len({t.device for t in named.values()}) != 1:
            raise ValueError(f"{who}: the tensors are on different devices")
        B, H, W = api.raft_check_gru(h.shape, [t.shape for t in segs], [w.shape for w in weights], [b.shape for b in biases])
        h = h.detach().contiguous()
        segs = [t.detach().contiguous() for t in segs]
        weights = [w.detach().contiguous() for w in weights]
        biases = [b.detach().contiguous() for b in biases]
        out = torch.empty((B, api.GRU_HIDDEN, H, W), dtype=torch.float32, device=h.device)
        seg_table = (C.c_void_p * len(segs))(*[t.data_ptr() for t in segs])
        seg_channels = (C.c_int32 * len(segs))(*[t.shape[1] for t in segs])
        w_table = (C.c_void_p * 6)(*[t.data_ptr() for t in weights])
        b_table = (C.c_void_p * 6)(*[t.data_ptr() for t in biases])
        _call(h.device, "raft_sepconv_gru_device", C.c_int32(B), C.c_int32(H), C.c_int32(W), tc.ptr(h), C.c_int32(len(segs)),
              seg_table, seg_channels, w_table, b_table, tc.ptr(out))
        return out


def _check_forward(who, named):
    """SepConvGRU's rules for a dict of named tensors: GPU, float32, no grad wanted, one device."""
    for name, t in named.items():
        if not (torch.is_tensor(t) and t.is_cuda):
            raise ValueError(f"{who} runs on GPU tensors: {name} is not on a GPU (there is no CPU path)")
        if t.dtype != torch.float32:
            raise TypeError(f"{who}: {name} must be float32 (got {t.dtype})")
        if torch.is_grad_enabled() and t.requires_grad:
            raise ValueError(f"{who} is forward only: {name} requires grad (call it under torch.no_grad())")
    if len({t.device for t in named.values()}) != 1:
        raise ValueError(f"{who}: the tensors are on different devices")


def _conv2d(who, segs, convs, relu, scale=1.0, out=None, out_first=0):
    """One launch of csrc/cvd_raftconv.h: the tensors `segs` (never concatenated) through one Conv2d module or two stacked along
    the output channels, into a new tensor or the channels out_first .. of `out`."""
    named = {f"x[{i}]": t for i, t in enumerate(segs)}
    for i, m in enumerate(convs):
        named[f"weight[{i}]"], named[f"bias[{i}]"] = m.weight, m.bias
    if out is not None:
        named["out"] = out
    _check_forward(who, named)
    for m in convs:
        api.raft_check_conv2d([t.shape for t in segs], [m.weight.shape], [m.bias.shape], stride=m.stride, dilation=m.dilation,
                              groups=m.groups)
    B, H, W, N = api.raft_check_conv2d([t.shape for t in segs], [m.weight.shape for m in convs], [m.bias.shape for m in convs],
                                       None if out is None else out.shape[1], out_first)
    segs = [t.detach().contiguous() for t in segs]
    weights = [m.weight.detach().contiguous() for m in convs]
    biases = [m.bias.detach().contiguous() for m in convs]
    if out is None:
        out = torch.empty((B, N, H, W), dtype=torch.float32, device=segs[0].device)
    elif not out.is_contiguous() or (out.shape[0], out.shape[2], out.shape[3]) != (B, H, W):
        raise ValueError(f"{who}: out must be a contiguous ({B}, C, {H}, {W}) tensor (got {tuple(out.shape)})")
    _call(out.device, "raft_conv2d_device", C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(len(segs)),
          (C.c_void_p * len(segs))(*[t.data_ptr() for t in segs]), (C.c_int32 * len(segs))(*[t.shape[1] for t in segs]),
          C.c_int32(len(weights)), (C.c_void_p * len(weights))(*[t.data_ptr() for t in weights]),
          (C.c_void_p * len(biases))(*[t.data_ptr() for t in biases]), C.c_int32(weights[0].shape[1]), C.c_int32(weights[0].shape[0]),
          C.c_int32(weights[0].shape[2]), C.c_int32(1), C.c_int32(1), C.c_int32(1), C.c_int32(1 if relu else 0), C.c_float(scale),
          tc.ptr(out), C.c_int32(out.shape[1]), C.c_int32(out_first))
    return out


def _segments(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


class FlowHead(torch.nn.Module):
    """The reference's FlowHead (raft/core/update.py:8-16): conv2(relu(conv1(x))), two launches of csrc/cvd_raftconv.h."""

    def __init__(self, input_dim=128, hidden_dim=256):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(input_dim, hidden_dim, 3, padding=1)
        self.conv2 = torch.nn.Conv2d(hidden_dim, 2, 3, padding=1)

    def forward(self, x):
        return _conv2d("FlowHead", (_conv2d("FlowHead", _segments(x), (self.conv1,), True),), (self.conv2,), False)


class BasicMotionEncoder(torch.nn.Module):
    """The reference's BasicMotionEncoder (raft/core/update.py:96-114): five launches of csrc/cvd_raftconv.h, the two cat replaced
    by channel windows of the outputs (the last launch also copies flow into channels 126..127 when it runs inside the block; on
    its own this module copies it with torch).  args: corr_levels and corr_radius are read (default 4, 4)."""

    def __init__(self, args=None):
        super().__init__()
        cor_planes = getattr(args, "corr_levels", 4) * (2 * getattr(args, "corr_radius", 4) + 1) ** 2
        self.convc1 = torch.nn.Conv2d(cor_planes, 256, 1, padding=0)
        self.convc2 = torch.nn.Conv2d(256, 192, 3, padding=1)
        self.convf1 = torch.nn.Conv2d(2, 128, 7, padding=3)
        self.convf2 = torch.nn.Conv2d(128, 64, 3, padding=1)
        self.conv = torch.nn.Conv2d(64 + 192, 128 - 2, 3, padding=1)

    def forward(self, flow, corr):
        who = "BasicMotionEncoder"
        _check_forward(who, {"flow": flow, "corr": corr})
        if flow.dim() != 4 or corr.dim() != 4 or flow.shape[1] != 2:
            raise ValueError(f"{who}: flow must be (B, 2, H, W) and corr (B, C, H, W) (got {tuple(flow.shape)}, {tuple(corr.shape)})")
        B, _, H, W = flow.shape
        cor_flo = torch.empty((B, 256, H, W), dtype=torch.float32, device=flow.device)
        out = torch.empty((B, 128, H, W), dtype=torch.float32, device=flow.device)
        _conv2d(who, (_conv2d(who, (corr,), (self.convc1,), True),), (self.convc2,), True, out=cor_flo, out_first=0)
        _conv2d(who, (_conv2d(who, (flow,), (self.convf1,), True),), (self.convf2,), True, out=cor_flo, out_first=192)
        _conv2d(who, (cor_flo,), (self.conv,), True, out=out, out_first=0)
        out[:, 126:] = flow.detach()
        return out


class BasicUpdateBlock(torch.nn.Module):
    """The reference's BasicUpdateBlock(args, hidden_dim=128, input_dim=128) (raft/core/update.py:133-156) with its parameter names
    and shapes (encoder.convc1 .. gru.convq2, flow_head.conv1 / conv2, mask.0 / mask.2), so the update_block.* part of a RAFT
    state dict loads unchanged.  forward(net, inp, corr, flow) -> (net, mask, delta_flow) is ONE call of the library: 8 launches
    of csrc/cvd_raftconv.h beside the 4 of the GRU, no cat, enqueued on the current stream without a host wait.
    compute_mask=False returns None for the mask and skips mask.0 and mask.2 (7 launches).  Forward only, float32, GPU tensors; the
    results are new tensors.  The scratch is the device handle's: calls on one device are ordered on one stream."""

    def __init__(self, args=None, hidden_dim=128, input_dim=128):
        super().__init__()
        if (hidden_dim, input_dim) != (api.GRU_HIDDEN, 128):
            raise ValueError(f"BasicUpdateBlock: hidden_dim = {api.GRU_HIDDEN} and input_dim = 128 are the only sizes of the kernels "
                             f"(RAFT's); got {hidden_dim}, {input_dim}")
        self.args = args
        self.encoder = BasicMotionEncoder(args)
        self.gru = SepConvGRU(hidden_dim=hidden_dim, input_dim=128 + hidden_dim)
        self.flow_head = FlowHead(hidden_dim, hidden_dim=256)
        self.mask = torch.nn.Sequential(torch.nn.Conv2d(128, 256, 3, padding=1), torch.nn.ReLU(inplace=True),
                                        torch.nn.Conv2d(256, 64 * 9, 1, padding=0))

    def forward(self, net, inp, corr, flow, upsample=True, compute_mask=True):
        who = "BasicUpdateBlock"
        modules = [self.get_submodule(n) for n in api.UPDATE_BLOCK_PARAMETERS]
        weights, biases = [m.weight for m in modules], [m.bias for m in modules]
        named = {"net": net, "inp": inp, "corr": corr, "flow": flow,
                 **{f"{n}.weight": w for n, w in zip(api.UPDATE_BLOCK_PARAMETERS, weights)},
                 **{f"{n}.bias": b for n, b in zip(api.UPDATE_BLOCK_PARAMETERS, biases)}}
        _check_forward(who, named)
        B, H, W = api.raft_check_update_block(net.shape, inp.shape, corr.shape, flow.shape, [w.shape for w in weights],
                                              [b.shape for b in biases])
        net, inp, corr, flow = (t.detach().contiguous() for t in (net, inp, corr, flow))
        weights = [w.detach().contiguous() for w in weights]
        biases = [b.detach().contiguous() for b in biases]
        dev = net.device
        net_out = torch.empty((B, api.GRU_HIDDEN, H, W), dtype=torch.float32, device=dev)
        delta_flow = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
        mask = torch.empty((B, 576, H, W), dtype=torch.float32, device=dev) if compute_mask else None
        _call(dev, "raft_update_block_device", C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(corr.shape[1]),
              C.c_int32(weights[0].shape[1]), tc.ptr(net), tc.ptr(inp), tc.ptr(corr), tc.ptr(flow),
              (C.c_void_p * 15)(*[t.data_ptr() for t in weights]), (C.c_void_p * 15)(*[t.data_ptr() for t in biases]),
              tc.ptr(net_out), tc.ptr(delta_flow), tc.ptr(mask) if compute_mask else None)
        return net_out, mask, delta_flow


def _make_norm(who, norm_fn, planes):
    """The reference's norm module of a layer, for its parameter and buffer names; its forward is never called."""
    if norm_fn == "batch":
        return torch.nn.BatchNorm2d(planes)
    if norm_fn == "instance":
        return torch.nn.InstanceNorm2d(planes)
    if norm_fn == "none":
        return torch.nn.Sequential()
    raise ValueError(f"{who}: norm_fn must be 'instance', 'batch' or 'none' (got {norm_fn!r}; group norm has no kernel)")


def _norm_vectors(who, norm):
    """(the four vectors of an eval BatchNorm2d in api.ENCODER_NORM_VECTORS order, eps); ValueError in training mode."""
    if norm.training:
        raise ValueError(f"{who}: batch norm in training mode has no kernel: call .eval() (or RAFT.freeze_bn())")
    if not norm.affine or not norm.track_running_stats:
        raise ValueError(f"{who}: the batch norm must have affine parameters and running statistics")
    return [norm.weight, norm.bias, norm.running_mean, norm.running_var], float(norm.eps)


def _encoder_conv(who, x, conv, norm, relu, residual=None):
    """One convolution of csrc/cvd_raftenc.h with what follows it in the reference: conv, `norm` (a BatchNorm2d in eval mode: fused;
    an InstanceNorm2d: the two launches behind, in place; an empty Sequential: nothing), ReLU, relu(residual + y)."""
    named = {"x": x, "weight": conv.weight, "bias": conv.bias}
    if residual is not None:
        named["residual"] = residual
    vectors, eps = None, 1e-5
    if isinstance(norm, torch.nn.BatchNorm2d):
        vectors, eps = _norm_vectors(who, norm)
        named.update({f"norm.{n}": v for n, v in zip(api.ENCODER_NORM_VECTORS, vectors)})
    instance = isinstance(norm, torch.nn.InstanceNorm2d)
    if instance:
        eps = float(norm.eps)
    _check_forward(who, named)
    for name, v in (("dilation", conv.dilation), ("groups", conv.groups)):
        if v not in (1, (1, 1)):
            raise ValueError(f"{who}: {name} must be 1 (got {v})")
    if tuple(conv.padding) != (conv.kernel_size[0] // 2,) * 2:
        raise ValueError(f"{who}: padding must be kernel_size // 2 (got {conv.padding})")
    B, H, W, Cin, N, k, Ho, Wo = api.raft_check_encoder_conv(x.shape, conv.weight.shape, conv.bias.shape, tuple(conv.stride),
                                                             None if vectors is None else [v.shape for v in vectors], eps,
                                                             None if residual is None else residual.shape)
    if instance:
        api.raft_check_instance_norm((B, N, Ho, Wo), eps)
    x = x.detach().contiguous()
    residual = None if residual is None else residual.detach().contiguous()
    weight, bias = conv.weight.detach().contiguous(), conv.bias.detach().contiguous()
    vectors = None if vectors is None else [v.detach().contiguous() for v in vectors]
    out = torch.empty((B, N, Ho, Wo), dtype=torch.float32, device=x.device)
    fused = not instance
    _call(x.device, "raft_encoder_conv_device", C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(Cin), C.c_int32(N), C.c_int32(k),
          C.c_int32(conv.stride[0]), tc.ptr(x), tc.ptr(weight), tc.ptr(bias),
          None if vectors is None else (C.c_void_p * 4)(*[v.data_ptr() for v in vectors]), C.c_float(eps),
          C.c_int32(1 if relu and fused else 0), tc.ptr(residual) if fused else None, tc.ptr(out))
    if instance:
        _call(x.device, "raft_instance_norm_device", C.c_int32(B), C.c_int32(N), C.c_int32(Ho), C.c_int32(Wo), tc.ptr(out), C.c_float(eps),
              C.c_int32(1 if relu else 0), tc.ptr(residual), tc.ptr(out))
    return out


class ResidualBlock(torch.nn.Module):
    """The reference's ResidualBlock (raft/core/extractor.py:8-60) with its module, parameter and buffer names (norm3 is also
    downsample.1, as there), on csrc/cvd_raftenc.h: relu(x' + relu(norm2(conv2(relu(norm1(conv1(x))))))), x' = x
    or norm3(downsample.0(x)) under stride 2.  Two or three convolution launches with the batch norm, ReLU and residual fused; the
    instance norm is two more launches behind each.  norm_fn: 'instance', 'batch' (eval mode only) or 'none'; 'group' is refused.
    BottleneckBlock is out of scope."""

    def __init__(self, in_planes, planes, norm_fn="group", stride=1):
        super().__init__()
        who = "ResidualBlock"
        if stride not in api.ENCODER_STRIDES:
            raise ValueError(f"{who}: stride must be 1 or 2 (got {stride})")
        self.conv1 = torch.nn.Conv2d(in_planes, planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = torch.nn.Conv2d(planes, planes, kernel_size=3, padding=1)
        self.relu = torch.nn.ReLU(inplace=True)
        self.norm1 = _make_norm(who, norm_fn, planes)
        self.norm2 = _make_norm(who, norm_fn, planes)
        self.downsample = None
        if stride != 1:
            self.norm3 = _make_norm(who, norm_fn, planes)
            self.downsample = torch.nn.Sequential(torch.nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride), self.norm3)

    def forward(self, x):
        who = "ResidualBlock"
        y = _encoder_conv(who, x, self.conv1, self.norm1, True)
        if self.downsample is not None:
            x = _encoder_conv(who, x, self.downsample[0], self.norm3, False)
        return _encoder_conv(who, y, self.conv2, self.norm2, True, residual=x)


class BasicEncoder(torch.nn.Module):
    """The reference's BasicEncoder (raft/core/extractor.py:124-197) with its module, parameter and buffer names, so the fnet.* and
    cnet.* parts of a RAFT state dict load unchanged.  forward(x), x a [B, 3, H, W] tensor scaled to [-1, 1] or a list of two (the
    list is returned as two tensors, like the reference's), is ONE call of the library (cvd_raft_encoder_device):
    16 convolution launches with bias, eval batch norm, ReLU and residual fused, and under instance norm two more launches behind
    each of the first fifteen.  A list is concatenated along the batch with one torch.cat of the two images (the reference does the
    same); the two results are views of the one output.  Forward only, float32, GPU tensors, eval mode: norm_fn='group', batch norm
    in training mode and dropout > 0 in training mode are refused (ValueError) before any device work.  The scratch is the device
    handle's: calls on one device are ordered on one stream.  SmallEncoder and BottleneckBlock are out of scope."""

    def __init__(self, output_dim=128, norm_fn="batch", dropout=0.0):
        super().__init__()
        who = "BasicEncoder"
        self.norm_fn = norm_fn
        self.norm1 = _make_norm(who, norm_fn, 64)
        self.conv1 = torch.nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3)
        self.relu1 = torch.nn.ReLU(inplace=True)
        self.layer1 = torch.nn.Sequential(ResidualBlock(64, 64, norm_fn, 1), ResidualBlock(64, 64, norm_fn, 1))
        self.layer2 = torch.nn.Sequential(ResidualBlock(64, 96, norm_fn, 2), ResidualBlock(96, 96, norm_fn, 1))
        self.layer3 = torch.nn.Sequential(ResidualBlock(96, 128, norm_fn, 2), ResidualBlock(128, 128, norm_fn, 1))
        self.conv2 = torch.nn.Conv2d(128, output_dim, kernel_size=1)
        self.dropout = torch.nn.Dropout2d(p=dropout) if dropout > 0 else None
        # the reference's initialisation (the norms' weight 1 and bias 0 are torch's defaults)
        for m in self.modules():
            if isinstance(m, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def check_mode(self):
        """ValueError where the module's mode has no kernel: dropout or a batch norm in training mode."""
        who = "BasicEncoder"
        if self.training and self.dropout is not None:
            raise ValueError(f"{who}: dropout in training mode has no kernel: call .eval()")
        for m in self.modules():
            if isinstance(m, torch.nn.BatchNorm2d) and m.training:
                raise ValueError(f"{who}: batch norm in training mode has no kernel: call .eval() (or RAFT.freeze_bn())")

    def forward(self, x):
        who = "BasicEncoder"
        is_list = isinstance(x, (tuple, list))
        images = list(x) if is_list else [x]
        if is_list and len(images) != 2:
            raise ValueError(f"{who}: a list input must hold two tensors (got {len(images)})")
        self.check_mode()
        convs = [self.get_submodule(n) for n in api.ENCODER_PARAMETERS]
        weights, biases = [m.weight for m in convs], [m.bias for m in convs]
        named = {**{f"x[{i}]": t for i, t in enumerate(images)},
                 **{f"{n}.weight": w for n, w in zip(api.ENCODER_PARAMETERS, weights)},
                 **{f"{n}.bias": b for n, b in zip(api.ENCODER_PARAMETERS, biases)}}
        norms, eps = None, 1e-5
        if self.norm_fn == "batch":
            norms = []
            for n in api.ENCODER_NORMS:
                vectors, eps = _norm_vectors(f"{who}: {n}", self.get_submodule(n))
                norms.append(vectors)
                named.update({f"{n}.{v}": t for v, t in zip(api.ENCODER_NORM_VECTORS, vectors)})
        elif self.norm_fn == "instance":
            eps = float(self.norm1.eps)
        _check_forward(who, named)
        if any(t.dim() != 4 or t.shape != images[0].shape for t in images):
            raise ValueError(f"{who}: the images must be (B, 3, H, W) alike (got {[tuple(t.shape) for t in images]})")
        batch = images[0].shape[0]
        shape = (batch * len(images),) + tuple(images[0].shape[1:])
        B, H, W, output_dim, mode, (h, w) = api.raft_check_encoder(
            shape, [t.shape for t in weights], [t.shape for t in biases], self.norm_fn,
            None if norms is None else [[t.shape for t in four] for four in norms], eps)
        x = torch.cat([t.detach() for t in images], 0) if is_list else images[0].detach()
        x = x.contiguous()
        weights = [t.detach().contiguous() for t in weights]
        biases = [t.detach().contiguous() for t in biases]
        table = None
        if norms is not None:
            flat = [t.detach().contiguous() for four in norms for t in four]
            table = (C.c_void_p * 60)(*[t.data_ptr() for t in flat])
        out = torch.empty((B, output_dim, h, w), dtype=torch.float32, device=x.device)
        _call(x.device, "raft_encoder_device", C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(output_dim), C.c_int32(mode),
              C.c_float(eps), tc.ptr(x), (C.c_void_p * 16)(*[t.data_ptr() for t in weights]),
              (C.c_void_p * 16)(*[t.data_ptr() for t in biases]), table, tc.ptr(out))
        return torch.split(out, [batch, batch], dim=0) if is_list else out


class RAFT(torch.nn.Module):
    """The reference's RAFT (raft/core/raft.py) without `small`, with its module, parameter and buffer names: the state dict has the
    reference's 179 keys in its order, so a checkpoint loads with strict=True, also through torch.nn.DataParallel(RAFT(args)).module
    as the reference loads it.  `from robust_cvd_amd.raft_ops import RAFT` is the whole integration.

    forward(image1, image2, iters=12, flow_init=None, upsample=True, test_mode=False), images [B, 3, H, W] in 0..255, returns what
    the reference returns: (flow at 1/8, upsampled flow) under test_mode, else the list of the upsampled flow of every iteration.
    Everything runs on the library: fnet on both images in one encoder call, CorrBlock, cnet, and per
    iteration the lookup, BasicUpdateBlock and upsample_flow; the image scaling, tanh / relu of the context split and the coordinate
    adds stay torch ops.  Under test_mode only the last iteration computes the mask and the upsampling (the same bits: the earlier
    masks are never read).  Forward only, float32, GPU tensors, batch norm in eval mode (.eval() or freeze_bn()); H and W multiples
    of 8 and at least 128 (the four-level pyramid needs 16 x 16 features).  args.small is refused: SmallEncoder, BottleneckBlock and
    SmallUpdateBlock are out of scope."""

    def __init__(self, args):
        super().__init__()
        if getattr(args, "small", False):
            raise ValueError("RAFT: args.small has no kernels (SmallEncoder and SmallUpdateBlock are out of scope)")
        self.args = args
        self.hidden_dim = hdim = 128
        self.context_dim = cdim = 128
        args.corr_levels = 4
        args.corr_radius = 4
        dropout = getattr(args, "dropout", 0)
        args.dropout = dropout
        self.fnet = BasicEncoder(output_dim=256, norm_fn="instance", dropout=dropout)
        self.cnet = BasicEncoder(output_dim=hdim + cdim, norm_fn="batch", dropout=dropout)
        self.update_block = BasicUpdateBlock(args, hidden_dim=hdim)

    def freeze_bn(self):
        for m in self.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eval()

    def forward(self, image1, image2, iters=12, flow_init=None, upsample=True, test_mode=False):
        who = "RAFT"
        named = {"image1": image1, "image2": image2}
        if flow_init is not None:
            named["flow_init"] = flow_init
        _check_forward(who, named)
        if image1.dim() != 4 or image1.shape[1] != 3 or image1.shape != image2.shape:
            raise ValueError(f"{who}: image1 and image2 must be (B, 3, H, W) alike (got {tuple(image1.shape)}, {tuple(image2.shape)})")
        B, _, H, W = image1.shape
        if H % 8 or W % 8:
            raise ValueError(f"{who}: height and width must be multiples of 8 (got {H} x {W}; pad the images as the reference's InputPadder does)")
        h, w = H // 8, W // 8
        if min(h, w) < 16:
            raise ValueError(f"{who}: {H} x {W} images give {h} x {w} features; the four-level correlation pyramid needs 16 x 16")
        if flow_init is not None and tuple(flow_init.shape) != (B, 2, h, w):
            raise ValueError(f"{who}: flow_init must be {(B, 2, h, w)} (got {tuple(flow_init.shape)})")
        if int(iters) < 1:
            raise ValueError(f"{who}: iters must be >= 1 (got {iters})")
        if any(p.device != image1.device for p in self.parameters()):
            raise ValueError(f"{who}: the parameters and the images are on different devices")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise ValueError(f"{who} is forward only: its parameters require grad (call it under torch.no_grad())")
        self.fnet.check_mode()
        self.cnet.check_mode()
        image1 = (2 * (image1 / 255.0) - 1.0).contiguous()
        image2 = (2 * (image2 / 255.0) - 1.0).contiguous()
        fmap1, fmap2 = self.fnet([image1, image2])
        corr_fn = CorrBlock(fmap1, fmap2, radius=self.args.corr_radius)
        cnet = self.cnet(image1)
        net, inp = torch.split(cnet, [self.hidden_dim, self.context_dim], dim=1)
        net = torch.tanh(net).contiguous()
        inp = torch.relu(inp).contiguous()
        ys, xs = torch.meshgrid(torch.arange(h, device=image1.device), torch.arange(w, device=image1.device), indexing="ij")
        coords0 = torch.stack([xs, ys], dim=0).float()[None].repeat(B, 1, 1, 1)
        coords1 = coords0.clone()
        if flow_init is not None:
            coords1 = coords1 + flow_init
        flow_predictions = []
        flow_up = None
        for it in range(int(iters)):
            corr = corr_fn(coords1)
            flow = coords1 - coords0
            wanted = not test_mode or it == int(iters) - 1
            net, up_mask, delta_flow = self.update_block(net, inp, corr, flow, compute_mask=wanted)
            coords1 = coords1 + delta_flow
            if wanted:
                flow_up = upsample_flow(coords1 - coords0, up_mask)
                flow_predictions.append(flow_up)
        if test_mode:
            return coords1 - coords0, flow_up
        return flow_predictions


def upsample_flow(flow, mask):
    """[N, 2, H, W] -> [N, 2, 8 H, 8 W]: the convex combination of the 3 x 3 neighbours of 8 flow under softmax(mask)."""
    _check("upsample_flow", flow=flow, mask=mask)
    N, H, W = api.raft_check_upsample(flow.shape, mask.shape)
    flow, mask = flow.detach().contiguous(), mask.detach().contiguous()
    out = torch.empty((N, 2, 8 * H, 8 * W), dtype=torch.float32, device=flow.device)
    _call(flow.device, "raft_upsample_flow_device", C.c_int32(N), C.c_int32(H), C.c_int32(W), tc.ptr(flow), tc.ptr(mask), tc.ptr(out))
    return out
