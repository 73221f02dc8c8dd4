"""What the torch drop-ins of the fine-tuning losses share (consistency.py, scene_flow.py, spatial_losses.py): the per-device
library handle, the checks and conversions of their tensor arguments, and the autograd function around one enqueued call of a
`*_device` entry point.

One `api.Solver` handle per device index serves every loss module of the process, so two modules (or two instances of one) on a
device also share that operator's scratch buffers: calls on one device are ordered on one stream, or synchronised across
streams ("device entry points").
"""
import ctypes as C

import torch

from . import api

_solvers = {}


def solver(device):
    """The process's handle of `device` (created at the first call)."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    if index not in _solvers:
        _solvers[index] = api.Solver(index)
    return _solvers[index]


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def check_depths(who, depths):
    if not (torch.is_tensor(depths) and depths.is_cuda):
        raise ValueError(f"{who} runs on GPU tensors: depths is not on a GPU (there is no CPU path)")
    if depths.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{who}: depths must be float32 or float64 (got {depths.dtype})")


def table(who, t, shape, name, like):
    """`t` detached, contiguous, as `shape`, on the device and in the dtype of `like` (no copy for a contiguous tensor of that
    dtype)."""
    if not (torch.is_tensor(t) and t.device == like.device):
        raise ValueError(f"{who}: {name} is not a tensor on {like.device}")
    return t.detach().to(like.dtype).reshape(shape).contiguous()


def scaled_warp(who, warp, F, H, W, like):
    """metadata["warp"] (normalised units) as pixel offsets [F, 2, H, W].  The reference scales its tensor in place, on every
    call; here a copy, the caller's tensor stays as it is."""
    scale = torch.tensor([W / 2, H / 2], dtype=like.dtype, device=like.device).view(1, 2, 1, 1)
    return table(who, warp, (F, 2, H, W), "warp", like) * scale


class EnqueuedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, name, num_results, arguments):
        """One call of the entry point `name`, enqueued on torch's current stream with no host synchronisation.  table [F, H, W]
        contiguous: the depths.  The call writes num_results doubles, the total first; arguments(result, grad) returns what the
        entry point takes between the handle and the stream, with result(k) the address of the k-th double and grad the address of
        the gradient table or None.  Returns (total in the table's dtype, the other results float64, detached).  The gradient
        table is computed by the same call when `table` needs it and kept for backward."""
        out = torch.empty(num_results, dtype=torch.float64, device=table.device)
        grad = torch.empty_like(table) if table.requires_grad else None
        handle = solver(table.device)
        with torch.cuda.device(table.device):
            stream = torch.cuda.current_stream().cuda_stream
            handle._check(handle._fn(name)(handle._h, *arguments(lambda k: C.c_void_p(out.data_ptr() + 8 * k), ptr(grad)),
                                           C.c_void_p(stream)))
        ctx.grad_table = grad
        rest = out[1:]
        ctx.mark_non_differentiable(rest)
        return out[0].to(table.dtype), rest

    @staticmethod
    def backward(ctx, grad_total, _grad_rest):
        return ctx.grad_table * grad_total.to(ctx.grad_table.dtype), None, None, None
