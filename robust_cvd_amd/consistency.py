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

This is the only module of the package that imports torch.
"""
import ctypes as C

import torch

from . import api


class _ConsistencyFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, module, desc, arrays):
        """table [F, H, W] contiguous; returns (total, terms [P, 3] float64).  The gradient table is computed by the same call
        when `table` needs it and kept for backward."""
        need_grad = table.requires_grad
        P = desc.num_pairs
        out = torch.empty(1 + 3 * P, dtype=torch.float64, device=table.device)
        grad = torch.empty_like(table) if need_grad else None
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        ext, intr, warp, pairs, flow_ab, flow_ba, weight_ab, weight_ba = arrays
        solver = module._solver(table.device)
        with torch.cuda.device(table.device):
            stream = torch.cuda.current_stream().cuda_stream
            solver._check(solver._fn("consistency_loss_device")(
                solver._h, C.byref(desc), ptr(table), ptr(ext), ptr(intr), ptr(warp), ptr(pairs), ptr(flow_ab), ptr(flow_ba),
                ptr(weight_ab), ptr(weight_ba), ptr(out), C.c_void_p(out.data_ptr() + 8), ptr(grad), C.c_void_p(stream)))
        ctx.grad_table = grad
        terms = out[1:].view(P, 3)
        ctx.mark_non_differentiable(terms)
        return out[0].to(table.dtype), terms

    @staticmethod
    def backward(ctx, grad_total, _grad_terms):
        return ctx.grad_table * grad_total.to(ctx.grad_table.dtype), None, None, None


class ConsistencyLoss(torch.nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        if opt.distance_type_static not in api.DISTANCE_TYPES:
            raise KeyError(opt.distance_type_static)
        self._solvers = {}
        self._pairs = {}

    def _solver(self, device):
        index = device.index if device.index is not None else torch.cuda.current_device()
        if index not in self._solvers:
            self._solvers[index] = api.Solver(index)
        return self._solvers[index]

    def _pair_frames(self, B, device):
        key = (B, device)
        if key not in self._pairs:
            self._pairs[key] = torch.arange(2 * B, dtype=torch.int32, device=device).view(B, 2)
        return self._pairs[key]

    def forward(self, depths, metadata):
        opt = self.opt
        if not (torch.is_tensor(depths) and depths.is_cuda):
            raise ValueError("ConsistencyLoss runs on GPU tensors: depths is not on a GPU (there is no CPU path)")
        if depths.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"ConsistencyLoss: depths must be float32 or float64 (got {depths.dtype})")
        if depths.dim() != 4 or depths.shape[1] != 2:
            raise ValueError(f"ConsistencyLoss: depths must be (B, 2, H, W) (got {tuple(depths.shape)})")
        B, N, H, W = depths.shape
        dev, dt = depths.device, depths.dtype

        def arr(t, shape, name):
            if not (torch.is_tensor(t) and t.device == dev):
                raise ValueError(f"ConsistencyLoss: {name} is not a tensor on {dev}")
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
        geom = metadata["geometry_consistency"]
        flows = [arr(f, (B, 2, H, W), "flows") for f in geom["flows"]]
        masks = [arr(m, (B, H, W), "masks") for m in geom["masks"]]
        if len(flows) != 2 or len(masks) != 2:
            raise ValueError("ConsistencyLoss: flows and masks are pairs of tensors (one per direction)")
        lambdas = (opt.lambda_static_reprojection, opt.lambda_static_disparity, opt.lambda_static_depth_ratio)
        desc = api.consistency_desc(dt == torch.float64, B * N, B, H, W, opt.distance_type_static, opt.distance_scale,
                                    getattr(opt, "distance_alpha", 1.0), lambdas, warp is not None)
        arrays = (ext, intr, warp, self._pair_frames(B, dev), flows[0], flows[1], masks[0], masks[1])
        total, terms = _ConsistencyFunction.apply(table, self, desc, arrays)
        batch_losses = {name: terms[:, q].to(dt) for q, name in enumerate(api.CONSISTENCY_TERMS) if lambdas[q] > 0}
        return total, batch_losses
