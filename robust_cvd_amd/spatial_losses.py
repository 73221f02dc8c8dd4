"""Drop-ins for the reference's `loss/disparity_smooth_loss.py::DisparitySmoothLoss` and `loss/contrast_loss.py::ContrastLoss`
on GPU tensors: one HIP pass computes the value and the complete depth gradient (csrc/cvd_spatial.h) instead of
the chains of pad / slice / elementwise / reduction launches.

    from robust_cvd_amd.spatial_losses import ContrastLoss, DisparitySmoothLoss
    loss, batch_losses = DisparitySmoothLoss(opt)(images, depths)     # the reference's constructors and call signatures
    loss = ContrastLoss(opt)(depth_orig, depth_pred)
    loss.backward()                                                    # d loss / d depths

`opt` supplies lambda_disparity_smooth and sigma_color_grad (DisparitySmoothLoss), lambda_contrast_loss and
lambda_contrast_thresh (ContrastLoss).  `depths` / `depth_pred` / `depth_orig` are (B, N, H, W), `images` (B, N, 3, H, W), tensors
on one GPU, float32 or float64 (the dtype of the predicted depths picks the kernels; the other tensor is converted to it).  They
map to the kernels' tables with F = B N frames without a copy when contiguous; the call is enqueued on torch's current stream with
no host synchronisation.  `spatial_terms` runs both terms in ONE kernel call (robust_cvd_amd.joint_loss.JointLoss uses it).

Differences from the reference: nothing is printed (its ContrastLoss prints three device reductions per call, three host
synchronisations); `batch_losses` come back detached; gradients flow to the predicted depths only (not to the images or the
original depths); `opt.distance_type` is not read (the reference constructs a distance there and never uses it).

Import this module (torch) before anything loads libcvd_hip.so, as robust_cvd_amd.consistency.
"""
import ctypes as C

import torch

from . import api


class _SpatialFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, solver, desc, depth_orig, image):
        """table [F, H, W] contiguous; returns (total, smooth [B] float64, contrast).  The gradient table is computed by the same
        call when `table` needs it and kept for backward."""
        need_grad = table.requires_grad
        B = desc.num_frames // desc.frames_per_sample
        out = torch.empty(2 + B, dtype=torch.float64, device=table.device)      # total, contrast, smooth[B]
        grad = torch.empty_like(table) if need_grad else None
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with torch.cuda.device(table.device):
            stream = torch.cuda.current_stream().cuda_stream
            solver._check(solver._fn("spatial_losses_device")(
                solver._h, C.byref(desc), ptr(table), ptr(depth_orig), ptr(image), ptr(out), C.c_void_p(out.data_ptr() + 16),
                C.c_void_p(out.data_ptr() + 8), ptr(grad), C.c_void_p(stream)))
        ctx.grad_table = grad
        smooth, contrast = out[2:], out[1]
        ctx.mark_non_differentiable(smooth, contrast)
        return out[0].to(table.dtype), smooth, contrast

    @staticmethod
    def backward(ctx, grad_total, _grad_smooth, _grad_contrast):
        return ctx.grad_table * grad_total.to(ctx.grad_table.dtype), None, None, None, None


_solvers = {}


def _solver(device):
    index = device.index if device.index is not None else torch.cuda.current_device()
    if index not in _solvers:
        _solvers[index] = api.Solver(index)
    return _solvers[index]


def spatial_terms(depths, depth_orig=None, images=None, *, lambda_disparity_smooth=0.0, sigma_color_grad=1.0,
                  lambda_contrast_loss=0.0, contrast_thresh=1.05, who="spatial_terms"):
    """Both spatial terms of `depths` (B, N, H, W) in one kernel call: (total, smooth (B,), contrast), `total` attached to
    `depths`, the other two detached, all in the dtype of `depths`.  depth_orig (B, N, H, W) is read when lambda_contrast_loss
    > 0, images (B, N, 3, H, W) when lambda_disparity_smooth > 0."""
    if not (torch.is_tensor(depths) and depths.is_cuda):
        raise ValueError(f"{who} runs on GPU tensors: depths is not on a GPU (there is no CPU path)")
    if depths.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{who}: depths must be float32 or float64 (got {depths.dtype})")
    if depths.dim() != 4:
        raise ValueError(f"{who}: depths must be (B, N, H, W) (got {tuple(depths.shape)})")
    B, N, H, W = depths.shape
    dev, dt = depths.device, depths.dtype

    def arr(t, shape, name):
        if not (torch.is_tensor(t) and t.device == dev):
            raise ValueError(f"{who}: {name} is not a tensor on {dev}")
        if t.numel() != B * N * H * W * (3 if len(shape) == 4 else 1):
            raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected to view as {shape}")
        return t.detach().to(dt).reshape(shape).contiguous()     # (no copy for a contiguous tensor of this dtype)

    table = depths.contiguous().view(B * N, H, W)
    orig = arr(depth_orig, (B * N, H, W), "depth_orig") if lambda_contrast_loss > 0 else None
    image = arr(images, (B * N, 3, H, W), "images") if lambda_disparity_smooth > 0 else None
    desc = api.spatial_desc(dt == torch.float64, B * N, N, H, W, lambda_disparity_smooth, sigma_color_grad, lambda_contrast_loss,
                            contrast_thresh)
    total, smooth, contrast = _SpatialFunction.apply(table, _solver(dev), desc, orig, image)
    return total, smooth.to(dt), contrast.to(dt)


class DisparitySmoothLoss(torch.nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt

    def forward(self, images, depths):
        """images (B, N, 3, H, W), depths (B, N, H, W): (loss, {"disparity_smooth": (B,)})"""
        opt = self.opt
        total, smooth, _contrast = spatial_terms(depths, images=images, lambda_disparity_smooth=opt.lambda_disparity_smooth,
                                                 sigma_color_grad=opt.sigma_color_grad, who="DisparitySmoothLoss")
        return total, {"disparity_smooth": smooth}


class ContrastLoss(torch.nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt

    def forward(self, depth_orig, depth_pred):
        """depth_orig, depth_pred (B, N, H, W): the loss"""
        opt = self.opt
        total, _smooth, _contrast = spatial_terms(depth_pred, depth_orig=depth_orig, lambda_contrast_loss=opt.lambda_contrast_loss,
                                                  contrast_thresh=opt.lambda_contrast_thresh, who="ContrastLoss")
        return total
