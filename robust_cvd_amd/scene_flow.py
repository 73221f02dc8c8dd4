"""Drop-in for the reference's `loss/scene_flow_loss.py::SceneFlowLoss` on GPU tensors: one HIP forward pass and one HIP backward
pass (csrc/cvd_sceneflow.h) instead of the chain of grid_sample / baddbmm / elementwise launches.

    from robust_cvd_amd.scene_flow import SceneFlowLoss
    loss, batch_losses, scene_flow = SceneFlowLoss(opt)(depths, metadata)      # the reference's constructor and call signature
    loss.backward()                                                            # d loss / d depths

`opt` supplies distance_type_static, distance_type_smooth, distance_scale, distance_alpha, lambda_scene_flow_static,
lambda_smooth_reprojection / _disparity / _depth_ratio and recon.  `depths` is (B, N, H, W) with N = 6 (ref, target, ref - 1,
ref + 1, target - 1, target + 1) when a smooth lambda is > 0 and N = 2 or 6 with the static term alone; metadata["extrinsics"]
(B, N, 3, 4), metadata["intrinsics"] (B, N, 4), metadata["warp"] (anything that views as (B N, 2, H, W), normalised units; read
when opt.recon != "colmap"), metadata["geometry_consistency"]["flows"] / ["masks"] (two tensors each: (B, 2, H, W) /
(B, 1, H, W)) and metadata["temporal_smoothness"]["flows"] / ["masks"] / ["valid"] (four tensors each, and (B, 2, 1)) are tensors
on one GPU, float32 or float64 (the dtype of `depths` picks the kernels; other tensors are converted to it).  They map to the
kernels' table with F = B N frames, frame b N + k, pairs (b N, b N + 1) and neighbours b N + 2 .. b N + 5, without a copy when
contiguous; the call is enqueued on torch's current stream with no host synchronisation.

Differences from the reference: `scene_flow` is None unless the module is constructed with scene_flow_maps=True (the reference
copies its six visualisation maps to the host on every call; with the flag they come back as numpy arrays [B, 3, H, W] in the
reference's order, those of the parts whose lambdas are > 0); `batch_losses` come back detached; gradients flow to `depths` only;
metadata["warp"] is NOT scaled in place (this module scales a copy).

Import this module (torch) before anything loads libcvd_hip.so, as robust_cvd_amd.consistency.
"""
import ctypes as C

import torch

from . import api
from . import torch_common as tc


class SceneFlowLoss(torch.nn.Module):
    def __init__(self, opt, scene_flow_maps=False):
        super().__init__()
        self.opt = opt
        self.scene_flow_maps = bool(scene_flow_maps)
        for name in (opt.distance_type_static, opt.distance_type_smooth):
            if name not in api.DISTANCE_TYPES:
                raise KeyError(name)
        self._frames = {}

    def _frame_tables(self, B, N, device):
        key = (B, N, device)
        if key not in self._frames:
            base = torch.arange(B, dtype=torch.int32, device=device).view(B, 1) * N
            pairs = (base + torch.arange(2, dtype=torch.int32, device=device).view(1, 2)).contiguous()
            nbrs = (base + torch.arange(2, 6, dtype=torch.int32, device=device).view(1, 4)).contiguous() if N == 6 else None
            self._frames[key] = (pairs, nbrs)
        return self._frames[key]

    def forward(self, depths, metadata):
        opt = self.opt
        tc.check_depths("SceneFlowLoss", depths)
        lambdas = (opt.lambda_scene_flow_static, opt.lambda_smooth_reprojection, opt.lambda_smooth_disparity,
                   opt.lambda_smooth_depth_ratio)
        smooth = any(v > 0 for v in lambdas[1:])
        if depths.dim() != 4 or depths.shape[1] not in ((6,) if smooth else (2, 6)):
            raise ValueError(f"SceneFlowLoss: depths must be (B, {'6' if smooth else '2 or 6'}, H, W) (got {tuple(depths.shape)})")
        B, N, H, W = depths.shape
        dev, dt = depths.device, depths.dtype

        arr = lambda t, shape, name: tc.table("SceneFlowLoss", t, shape, name, depths)

        table = depths.contiguous().view(B * N, H, W)
        ext = arr(metadata["extrinsics"], (B * N, 3, 4), "extrinsics")
        intr = arr(metadata["intrinsics"], (B * N, 4), "intrinsics")
        warp = tc.scaled_warp("SceneFlowLoss", metadata["warp"], B * N, H, W, depths) if opt.recon != "colmap" else None
        flows = masks = nflows = nmasks = valid = None
        if lambdas[0] > 0:
            geom = metadata["geometry_consistency"]
            flows = [arr(f, (B, 2, H, W), "flows") for f in geom["flows"]]
            masks = [arr(m, (B, H, W), "masks") for m in geom["masks"]]
            if len(flows) != 2 or len(masks) != 2:
                raise ValueError("SceneFlowLoss: geometry_consistency flows and masks are pairs of tensors (one per direction)")
        if smooth:
            sm = metadata["temporal_smoothness"]
            nflows = [arr(f, (B, 2, H, W), "temporal_smoothness flows") for f in sm["flows"]]
            nmasks = [arr(m, (B, H, W), "temporal_smoothness masks") for m in sm["masks"]]
            if len(nflows) != 4 or len(nmasks) != 4:
                raise ValueError("SceneFlowLoss: temporal_smoothness flows and masks are four tensors each")
            valid = arr(sm["valid"], (B, 2), "temporal_smoothness valid")
        pairs, nbrs = self._frame_tables(B, N, dev)
        desc = api.scene_flow_desc(dt == torch.float64, B * N, B, H, W, opt.distance_type_static, opt.distance_type_smooth,
                                   opt.distance_scale, getattr(opt, "distance_alpha", 1.0), lambdas, warp is not None)
        # maps [6, B, 3, H, W]: the six visualisation maps, written by the same call on request
        maps = torch.empty((6, B, 3, H, W), dtype=dt, device=dev) if self.scene_flow_maps else None
        group = lambda ts: None if ts is None else (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        total, terms = tc.EnqueuedLoss.apply(table, "scene_flow_loss_device", 1 + 4 * B, lambda result, grad: (
            C.byref(desc), tc.ptr(table), tc.ptr(ext), tc.ptr(intr), tc.ptr(warp), tc.ptr(pairs), group(flows), group(masks),
            tc.ptr(nbrs if smooth else None), group(nflows), group(nmasks), tc.ptr(valid), result(0), result(1), grad, tc.ptr(maps)))
        terms = terms.view(B, 4)
        batch_losses = {name: terms[:, q].to(dt) for q, name in enumerate(api.SCENE_FLOW_TERMS) if lambdas[q] > 0}
        scene_flow = None
        if self.scene_flow_maps:
            host = maps.cpu().numpy()
            scene_flow = ([host[0], host[1]] if lambdas[0] > 0 else []) + ([host[k] for k in range(2, 6)] if smooth else [])
        return total, batch_losses, scene_flow
