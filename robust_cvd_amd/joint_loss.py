"""Drop-in for the reference's `loss/joint_loss.py::JointLoss` (and `loss/parameter_loss.py::ParameterLoss`), the criterion
`depth_fine_tuning.py` holds: this package's ConsistencyLoss, SceneFlowLoss (§3.11) and the two spatial terms
(§3.12) composed under the reference's `lambda` conditions.

    from robust_cvd_amd.joint_loss import JointLoss
    criterion = JointLoss(opt, parameters_init)                  # the reference's constructor and call signature
    loss, batch_losses, scene_flow = criterion(images, depths_orig, depths, metadata, parameters)
    loss.backward()

`images` (B, N, 3, H, W), `depths_orig` and `depths` (B, N, H, W) and the tensors of `metadata` (see consistency.py and
scene_flow.py) live on one GPU; N = 2, or 6 when a temporally smooth lambda is > 0.  With N = 6 the consistency term gets frames
0 and 1 of every sample (slices of depths, extrinsics, intrinsics and warp), as the reference's own loop over the two flow
directions does.  When both spatial terms are on they run in ONE kernel call.  ParameterLoss is plain torch
(lambda sum |p - p_init| over a list of arbitrary tensors; off by default); JointLoss(..., fused_parameter_loss=True) uses
robust_cvd_amd.parameter_loss.ParameterLoss instead: one launch over all tensors, and one for their gradients (DESIGN.md §3.13;
contiguous float32 / float64 parameters on one GPU).

Differences from the reference:
  * nothing is printed (the reference prints every term, one host synchronisation each);
  * `loss` has shape (1,) and the dtype and device of `depths` (the reference accumulates into a float32 tensor on its global
    device);
  * `batch_losses` of the kernel terms are detached, and gradients flow to `depths` (and `parameters`) only;
  * `scene_flow` is None unless the module is constructed with scene_flow_maps=True (scene_flow.py);
  * one quirk is NOT reproduced: when opt.recon != "colmap", both of the reference's geometric modules scale metadata["warp"]
    IN PLACE by (W / 2, H / 2), so with both on its scene-flow term sees a warp that has been scaled twice (and the caller's
    tensor changes on every call).  This package's modules scale copies: each term sees the warp scaled once.

Import this module (torch) before anything loads libcvd_hip.so, as robust_cvd_amd.consistency.
"""
import torch

from . import parameter_loss as fused
from .consistency import ConsistencyLoss
from .scene_flow import SceneFlowLoss
from .spatial_losses import ContrastLoss, DisparitySmoothLoss, spatial_terms


class ParameterLoss:
    def __init__(self, parameters_init, opt):
        self.parameters_init = parameters_init
        self.opt = opt
        assert opt.lambda_parameter > 0

    def __call__(self, parameters):
        diff = [torch.abs(p - pi.data) for p, pi in zip(parameters, self.parameters_init)]
        loss = self.opt.lambda_parameter * torch.sum(torch.cat([d.flatten() for d in diff]))
        return loss, {"parameter_loss": loss.reshape(1, -1)}


def _has_consistency(opt):
    return opt.lambda_static_disparity > 0 or opt.lambda_static_reprojection > 0 or opt.lambda_static_depth_ratio > 0


def _has_scene_flow(opt):
    return (opt.lambda_scene_flow_static > 0 or opt.lambda_smooth_reprojection > 0 or opt.lambda_smooth_disparity > 0
            or opt.lambda_smooth_depth_ratio > 0)


class JointLoss(torch.nn.Module):
    def __init__(self, opt, parameters_init=None, scene_flow_maps=False, fused_parameter_loss=False):
        super().__init__()
        self.opt = opt
        if opt.lambda_parameter > 0:
            assert parameters_init is not None
            self.parameter_loss = (fused.ParameterLoss if fused_parameter_loss else ParameterLoss)(parameters_init, opt)
        if _has_consistency(opt):
            self.consistency_loss = ConsistencyLoss(opt)
        if _has_scene_flow(opt):
            self.scene_flow_loss = SceneFlowLoss(opt, scene_flow_maps=scene_flow_maps)
        if opt.lambda_disparity_smooth > 0:
            self.disparity_smooth_loss = DisparitySmoothLoss(opt)
        if opt.lambda_contrast_loss > 0:
            self.contrast_loss = ContrastLoss(opt)

    def __call__(self, images, depths_orig, depths, metadata, parameters=None):
        opt = self.opt
        loss = torch.zeros(1, dtype=depths.dtype, device=depths.device)
        batch_losses = {}
        if opt.lambda_parameter > 0:
            assert parameters is not None
            para_loss, para_batch_losses = self.parameter_loss(parameters)
            loss = loss + para_loss.to(loss.dtype)
            batch_losses.update(para_batch_losses)
        if _has_consistency(opt):
            pair_depths, pair_meta = depths, metadata
            if depths.shape[1] != 2:     # frames 0 and 1 of every sample
                pair_depths = depths[:, :2]
                pair_meta = dict(metadata, extrinsics=metadata["extrinsics"][:, :2], intrinsics=metadata["intrinsics"][:, :2])
                if opt.recon != "colmap":
                    B, N, H, W = depths.shape
                    pair_meta["warp"] = metadata["warp"].reshape(B, N, 2, H, W)[:, :2]
            consis_loss, consis_batch_losses = self.consistency_loss(pair_depths, pair_meta)
            loss = loss + consis_loss
            batch_losses.update(consis_batch_losses)
        scene_flow = None
        if _has_scene_flow(opt):
            scene_flow_loss, scene_flow_batch_losses, scene_flow = self.scene_flow_loss(depths, metadata)
            loss = loss + scene_flow_loss
            batch_losses.update(scene_flow_batch_losses)
        smooth_on, contrast_on = opt.lambda_disparity_smooth > 0, opt.lambda_contrast_loss > 0
        if smooth_on and contrast_on:      # one kernel call for the pair
            spatial, smooth, _contrast = spatial_terms(
                depths, depths_orig, images, lambda_disparity_smooth=opt.lambda_disparity_smooth,
                sigma_color_grad=opt.sigma_color_grad, lambda_contrast_loss=opt.lambda_contrast_loss,
                contrast_thresh=opt.lambda_contrast_thresh, who="JointLoss")
            loss = loss + spatial
            batch_losses["disparity_smooth"] = smooth
        elif smooth_on:
            disparity_smooth_loss, disparity_smooth_batch_losses = self.disparity_smooth_loss(images, depths)
            loss = loss + disparity_smooth_loss
            batch_losses.update(disparity_smooth_batch_losses)
        elif contrast_on:
            loss = loss + self.contrast_loss(depths_orig, depths)
        return loss, batch_losses, scene_flow
