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


class _SceneFlowFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, module, desc, arrays, want_maps):
        """table [F, H, W] contiguous; returns (total, terms [P, 4] float64, maps [6, P, 3, H, W] or an empty tensor).  The gradient
        table is computed by the same call when `table` needs it and kept for backward."""
        need_grad = table.requires_grad
        P = desc.num_pairs
        F, H, W = table.shape
        out = torch.empty(1 + 4 * P, dtype=torch.float64, device=table.device)
        grad = torch.empty_like(table) if need_grad else None
        maps = torch.empty((6, P, 3, H, W) if want_maps else (0,), dtype=table.dtype, device=table.device)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        group = lambda ts: None if ts is None else (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        ext, intr, warp, pairs, flows, masks, nbrs, nflows, nmasks, valid = arrays
        solver = module._solver(table.device)
        with torch.cuda.device(table.device):
            stream = torch.cuda.current_stream().cuda_stream
            solver._check(solver._fn("scene_flow_loss_device")(
                solver._h, C.byref(desc), ptr(table), ptr(ext), ptr(intr), ptr(warp), ptr(pairs), group(flows), group(masks),
                ptr(nbrs), group(nflows), group(nmasks), ptr(valid), ptr(out), C.c_void_p(out.data_ptr() + 8), ptr(grad),
                ptr(maps) if want_maps else None, C.c_void_p(stream)))
        ctx.grad_table = grad
        terms = out[1:].view(P, 4)
        ctx.mark_non_differentiable(terms, maps)
        return out[0].to(table.dtype), terms, maps

    @staticmethod
    def backward(ctx, grad_total, _grad_terms, _grad_maps):
        return ctx.grad_table * grad_total.to(ctx.grad_table.dtype), None, None, None, None


class SceneFlowLoss(torch.nn.Module):
    def __init__(self, opt, scene_flow_maps=False):
        super().__init__()
        self.opt = opt
        self.scene_flow_maps = bool(scene_flow_maps)
        for name in (opt.distance_type_static, opt.distance_type_smooth):
            if name not in api.DISTANCE_TYPES:
                raise KeyError(name)
        self._solvers = {}
        self._frames = {}

    def _solver(self, device):
        index = device.index if device.index is not None else torch.cuda.current_device()
        if index not in self._solvers:
            self._solvers[index] = api.Solver(index)
        return self._solvers[index]

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
        if not (torch.is_tensor(depths) and depths.is_cuda):
            raise ValueError("SceneFlowLoss runs on GPU tensors: depths is not on a GPU (there is no CPU path)")
        if depths.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"SceneFlowLoss: depths must be float32 or float64 (got {depths.dtype})")
        lambdas = (opt.lambda_scene_flow_static, opt.lambda_smooth_reprojection, opt.lambda_smooth_disparity,
                   opt.lambda_smooth_depth_ratio)
        smooth = any(v > 0 for v in lambdas[1:])
        if depths.dim() != 4 or depths.shape[1] not in ((6,) if smooth else (2, 6)):
            raise ValueError(f"SceneFlowLoss: depths must be (B, {'6' if smooth else '2 or 6'}, H, W) (got {tuple(depths.shape)})")
        B, N, H, W = depths.shape
        dev, dt = depths.device, depths.dtype

        def arr(t, shape, name):
            if not (torch.is_tensor(t) and t.device == dev):
                raise ValueError(f"SceneFlowLoss: {name} is not a tensor on {dev}")
            t = t.detach().to(dt).reshape(shape)     # (no copy for a contiguous tensor of this dtype)
            return t.contiguous()

        table = depths.contiguous().view(B * N, H, W)
        ext = arr(metadata["extrinsics"], (B * N, 3, 4), "extrinsics")
        intr = arr(metadata["intrinsics"], (B * N, 4), "intrinsics")
        warp = None
        if opt.recon != "colmap":
            # the reference scales metadata["warp"] in place, on every call; here a copy, the caller's tensor stays as it is
            scale = torch.tensor([W / 2, H / 2], dtype=dt, device=dev).view(1, 2, 1, 1)
            warp = arr(metadata["warp"], (B * N, 2, H, W), "warp") * scale
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
        arrays = (ext, intr, warp, pairs, flows, masks, nbrs if smooth else None, nflows, nmasks, valid)
        total, terms, maps = _SceneFlowFunction.apply(table, self, desc, arrays, self.scene_flow_maps)
        batch_losses = {name: terms[:, q].to(dt) for q, name in enumerate(api.SCENE_FLOW_TERMS) if lambdas[q] > 0}
        scene_flow = None
        if self.scene_flow_maps:
            host = maps.cpu().numpy()
            scene_flow = ([host[0], host[1]] if lambdas[0] > 0 else []) + ([host[k] for k in range(2, 6)] if smooth else [])
        return total, batch_losses, scene_flow
