"""Drop-in for the reference's `loss/parameter_loss.py::ParameterLoss` on GPU tensors: lambda_parameter sum |p - p_init| over
every parameter tensor in ONE kernel launch, and one more for all the gradients (csrc/cvd_paramstep.h), instead
of a `sub` and an `abs` per tensor, a `cat` that copies the whole parameter set and a `sum`, and the same again backwards.

    from robust_cvd_amd.parameter_loss import ParameterLoss
    criterion = ParameterLoss(parameters_init, opt)              # the reference's constructor and call signature
    loss, batch_losses = criterion(model.parameters())            # any iterable of parameters: the reference passes a generator
    loss.backward()                                               # lambda sign(p - p_init) grad, sign(0) = 0 as torch.abs

The parameters are contiguous float32 or float64 tensors on one GPU (`parameters_init` is converted to their dtype and device
once); anything else raises ValueError / TypeError naming the tensor.  Tensors of both precisions may be mixed: one launch per
precision present.  The sum is formed in float64 and repeats bit for bit; `loss` has the parameters' dtype (float64 when both are
present).  The calls are enqueued on torch's current stream with no host synchronisation; the table of the tensor list is kept on
the handle and rebuilt only when the list changes, so alternating two lists of different shapes on one device costs a rebuild
(one stream wait) per call.

Import this module (torch) before anything loads libcvd_hip.so, as robust_cvd_amd.consistency.
"""
import ctypes as C

import torch

from . import api
from . import torch_common as tc

_PRECISIONS = (torch.float32, torch.float64)


def check_parameters(who, tensors, what="parameters"):
    """The device of a list of contiguous float32 / float64 GPU tensors (None for an empty list)."""
    device = None
    for i, t in enumerate(tensors):
        name = f"{what}[{i}]"
        if not torch.is_tensor(t):
            raise TypeError(f"{who}: {name} is not a tensor (got {type(t).__name__})")
        if not t.is_cuda:
            raise ValueError(f"{who} runs on GPU tensors: {name} is on {t.device} (there is no CPU path)")
        if t.dtype not in _PRECISIONS:
            raise TypeError(f"{who}: {name} must be float32 or float64 (got {t.dtype}; half precisions are not supported)")
        if t.is_sparse or not t.is_contiguous():
            raise ValueError(f"{who}: {name} of shape {tuple(t.shape)} is not contiguous")
        if device is None:
            device = t.device
        elif t.device != device:
            raise ValueError(f"{who}: {name} is on {t.device}, {what}[0] on {device}")
    return device


def by_precision(tensors):
    """{dtype: indices} of the precisions present, float32 first."""
    return {dt: idx for dt in _PRECISIONS for idx in [[i for i, t in enumerate(tensors) if t.dtype == dt]] if idx}


def addresses(tensors):
    return (C.c_void_p * max(len(tensors), 1))(*[t.data_ptr() for t in tensors])


def element_counts(tensors):
    return (C.c_int64 * max(len(tensors), 1))(*[t.numel() for t in tensors])


class _ParameterL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lam, inits, *params):
        device = params[0].device
        groups = by_precision(params)
        totals = torch.empty(len(groups), dtype=torch.float64, device=device)
        handle = tc.solver(device)
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for k, (dt, idx) in enumerate(groups.items()):
                p, p0 = [params[i] for i in idx], [inits[i] for i in idx]
                desc = api.param_desc(dt == torch.float64, len(idx))
                handle._check(handle._fn("parameter_l1_device")(
                    handle._h, C.byref(desc), addresses(p), addresses(p0), element_counts(p), C.c_double(lam),
                    C.c_void_p(totals.data_ptr() + 8 * k), None, None, C.c_int32(0), stream))
        ctx.lam, ctx.inits, ctx.groups = lam, inits, groups
        ctx.save_for_backward(*params)
        return totals.sum().to(torch.float64 if torch.float64 in groups else torch.float32)

    @staticmethod
    def backward(ctx, grad_total):
        params = ctx.saved_tensors
        device = params[0].device
        grads = [torch.empty_like(p) for p in params]     # (every tensor keeps its place in the table: the table stays the forward's)
        handle = tc.solver(device)
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for dt, idx in ctx.groups.items():
                p, p0, g = [params[i] for i in idx], [ctx.inits[i] for i in idx], [grads[i] for i in idx]
                scale = grad_total.detach().to(device=device, dtype=dt).reshape(1).contiguous()
                desc = api.param_desc(dt == torch.float64, len(idx))
                handle._check(handle._fn("parameter_l1_device")(
                    handle._h, C.byref(desc), addresses(p), addresses(p0), element_counts(p), C.c_double(ctx.lam), None,
                    addresses(g), tc.ptr(scale), C.c_int32(0), stream))
        return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


class ParameterLoss:
    def __init__(self, parameters_init, opt):
        self.parameters_init = [p.detach() for p in parameters_init]
        self.opt = opt
        assert opt.lambda_parameter > 0

    def __call__(self, parameters):
        """parameters: an iterable of tensors that match parameters_init: (loss, {"parameter_loss": loss.reshape(1, -1)})"""
        who = "ParameterLoss"
        params = list(parameters)
        inits = self.parameters_init
        if len(params) != len(inits):
            raise ValueError(f"{who}: {len(params)} parameters for {len(inits)} initial values")
        device = check_parameters(who, params)
        if not params:
            raise ValueError(f"{who}: the parameter list is empty")
        for i, (p, p0) in enumerate(zip(params, inits)):
            if not torch.is_tensor(p0) or p0.shape != p.shape:
                raise ValueError(f"{who}: parameters_init[{i}] does not have the shape {tuple(p.shape)} of parameters[{i}]")
            if p0.dtype != p.dtype or p0.device != p.device or not p0.is_contiguous():
                inits[i] = p0.to(device=device, dtype=p.dtype).contiguous()     # once
        loss = _ParameterL1.apply(float(self.opt.lambda_parameter), inits, *params)
        return loss, {"parameter_loss": loss.reshape(1, -1)}
