"""Drop-in for the reference's `loss/consistency_loss.py::ConsistencyLoss` on GPU tensors: one HIP forward pass and one HIP
backward pass (csrc/cvd_consistency.h) instead of the chain of elementwise / bmm / grid_sample launches.

    from robust_cvd_amd.consistency import ConsistencyLoss
    loss, batch_losses = ConsistencyLoss(opt)(depths, metadata)      # the reference's constructor and call signature
    loss.backward()                                                  # d loss / d depths

`opt` supplies distance_type_static, distance_scale, distance_alpha, lambda_static_reprojection / _disparity / _depth_ratio and
recon.  `depths` (B, 2, H, W), metadata["extrinsics"] (B, 2, 3, 4), metadata["intrinsics"] (B, 2, 4), metadata["warp"] (anything
that views as (2 B, 2, H, W), normalised units; read when opt.recon != "colmap") and metadata["geometry_consistency"]["flows"] /
["masks"] (two tensors each: (B, 2, H, W) / (B, 1, H, W)) are tensors on one GPU, float32 or float64 (the dtype of `depths`
picks the kernels; other tensors are converted to it).  They map to the kernels' table with F = 2 B frames and pairs
(2 b, 2 b + 1) without a copy when contiguous; the call is enqueued on torch's current stream with no host synchronisation.

Differences from the reference: `batch_losses` come back detached (the reference returns them attached to the graph; its
training loop only logs them), gradients flow to `depths` only (not to cameras or flows), and metadata["warp"] is NOT scaled in
place (the reference multiplies it by W/2, H/2 through a view on every call; this module scales a copy).

Import this module (torch) before anything loads libcvd_hip.so.  The handle, the tensor checks and the autograd function are those
of robust_cvd_amd.torch_common, shared with scene_flow.py and spatial_losses.py.
"""
import ctypes as C

import torch

from . import api
from . import torch_common as tc


class ConsistencyLoss(torch.nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        if opt.distance_type_static not in api.DISTANCE_TYPES:
            raise KeyError(opt.distance_type_static)
        self._pairs = {}

    def _pair_frames(self, B, device):
        key = (B, device)
        if key not in self._pairs:
            self._pairs[key] = torch.arange(2 * B, dtype=torch.int32, device=device).view(B, 2)
        return self._pairs[key]

    def forward(self, depths, metadata):
        opt = self.opt
        tc.check_depths("ConsistencyLoss", depths)
        if depths.dim() != 4 or depths.shape[1] != 2:
            raise ValueError(f"ConsistencyLoss: depths must be (B, 2, H, W) (got {tuple(depths.shape)})")
        B, N, H, W = depths.shape
        dev, dt = depths.device, depths.dtype

        arr = lambda t, shape, name: tc.table("ConsistencyLoss", t, shape, name, depths)

        table = depths.contiguous().view(B * N, H, W)
        ext = arr(metadata["extrinsics"], (B * N, 3, 4), "extrinsics")
        intr = arr(metadata["intrinsics"], (B * N, 4), "intrinsics")
        warp = tc.scaled_warp("ConsistencyLoss", metadata["warp"], B * N, H, W, depths) if opt.recon != "colmap" else None
        geom = metadata["geometry_consistency"]
        flows = [arr(f, (B, 2, H, W), "flows") for f in geom["flows"]]
        masks = [arr(m, (B, H, W), "masks") for m in geom["masks"]]
        if len(flows) != 2 or len(masks) != 2:
            raise ValueError("ConsistencyLoss: flows and masks are pairs of tensors (one per direction)")
        lambdas = (opt.lambda_static_reprojection, opt.lambda_static_disparity, opt.lambda_static_depth_ratio)
        desc = api.consistency_desc(dt == torch.float64, B * N, B, H, W, opt.distance_type_static, opt.distance_scale,
                                    getattr(opt, "distance_alpha", 1.0), lambdas, warp is not None)
        arrays = (table, ext, intr, warp, self._pair_frames(B, dev), flows[0], flows[1], masks[0], masks[1])
        total, terms = tc.EnqueuedLoss.apply(table, "consistency_loss_device", 1 + 3 * B, lambda result, grad: (
            C.byref(desc), *map(tc.ptr, arrays), result(0), result(1), grad))
        terms = terms.view(B, 3)
        batch_losses = {name: terms[:, q].to(dt) for q, name in enumerate(api.CONSISTENCY_TERMS) if lambdas[q] > 0}
        return total, batch_losses
