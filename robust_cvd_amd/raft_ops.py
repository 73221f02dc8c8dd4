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


def upsample_flow(flow, mask):
    """[N, 2, H, W] -> [N, 2, 8 H, 8 W]: the convex combination of the 3 x 3 neighbours of 8 flow under softmax(mask)."""
    _check("upsample_flow", flow=flow, mask=mask)
    N, H, W = api.raft_check_upsample(flow.shape, mask.shape)
    flow, mask = flow.detach().contiguous(), mask.detach().contiguous()
    out = torch.empty((N, 2, 8 * H, 8 * W), dtype=torch.float32, device=flow.device)
    _call(flow.device, "raft_upsample_flow_device", C.c_int32(N), C.c_int32(H), C.c_int32(W), tc.ptr(flow), tc.ptr(mask), tc.ptr(out))
    return out
