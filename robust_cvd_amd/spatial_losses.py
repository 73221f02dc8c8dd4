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
from . import torch_common as tc
from .torch_common import solver as _solver     # (the process's handle of a device, as before the modules shared it)


def spatial_terms(depths, depth_orig=None, images=None, *, lambda_disparity_smooth=0.0, sigma_color_grad=1.0,
                  lambda_contrast_loss=0.0, contrast_thresh=1.05, who="spatial_terms"):
    """Both spatial terms of `depths` (B, N, H, W) in one kernel call: (total, smooth (B,), contrast), `total` attached to
    `depths`, the other two detached, all in the dtype of `depths`.  depth_orig (B, N, H, W) is read when lambda_contrast_loss
    > 0, images (B, N, 3, H, W) when lambda_disparity_smooth > 0."""
    tc.check_depths(who, depths)
    if depths.dim() != 4:
        raise ValueError(f"{who}: depths must be (B, N, H, W) (got {tuple(depths.shape)})")
    B, N, H, W = depths.shape
    dev, dt = depths.device, depths.dtype

    def arr(t, shape, name):
        if torch.is_tensor(t) and t.device == dev and t.numel() != B * N * H * W * (3 if len(shape) == 4 else 1):
            raise ValueError(f"{who}: {name} has shape {tuple(t.shape)}, expected to view as {shape}")
        return tc.table(who, t, shape, name, depths)

    table = depths.contiguous().view(B * N, H, W)
    orig = arr(depth_orig, (B * N, H, W), "depth_orig") if lambda_contrast_loss > 0 else None
    image = arr(images, (B * N, 3, H, W), "images") if lambda_disparity_smooth > 0 else None
    desc = api.spatial_desc(dt == torch.float64, B * N, N, H, W, lambda_disparity_smooth, sigma_color_grad, lambda_contrast_loss,
                            contrast_thresh)
    # the results: total, contrast, smooth[B]
    total, rest = tc.EnqueuedLoss.apply(table, "spatial_losses_device", 2 + B, lambda result, grad: (
        C.byref(desc), tc.ptr(table), tc.ptr(orig), tc.ptr(image), result(0), result(2), result(1), grad))
    return total, rest[1:].to(dt), rest[0].to(dt)


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
