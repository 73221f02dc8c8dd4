"""Development aid (GPU): the consistency loss of flow pairs (cvd_consistency.h, the reference's ConsistencyLoss) through the
device entry point, in f32 and f64, at a training batch (B = 4 pairs of 384 x 224, 8 frames) and at the benchmarked video's
pair list (300 frames, 4140 pairs), l1 distance, lambdas (1, 0, 100), warp on, every weight 1.
  * kernel ms of the forward pass and of forward + backward: torch events around the enqueued call (inputs resident, no copies),
    median of --calls after warm-up;
  * algorithmic bytes against the HBM peak (8 TB/s): per (pair, direction, pixel) the six own values (depth, two flow components,
    weight, two warp components) and the target's depth once; the backward pass reads the same again, zeroes the gradient table
    and adds five values per sample with atomics (read + write);
  * the wall clock of one robust_cvd_amd.consistency.ConsistencyLoss call with .backward() at the batch size, host side included;
  * the same loss written in plain torch from the formulas of DESIGN.md §3.10 (l1, no disparity term), forward + backward, as the
    device baseline at the batch size.
Usage: python tools/consistency_bench.py [--calls 20] [--pairs 4140] [--frames 300]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # (before the library is loaded: the process then holds one HIP runtime)

from robust_cvd_amd import api, synth
from robust_cvd_amd.consistency import ConsistencyLoss

HBM_PEAK = 8.0e12


def make_inputs(F, pairs, H, W, dtype, device, seed=3):
    g = torch.Generator(device=device).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, device=device, dtype=dtype)
    P = len(pairs)
    yy, xx = torch.meshgrid(torch.arange(H, device=device, dtype=dtype), torch.arange(W, device=device, dtype=dtype), indexing="ij")
    depth = 3.0 + 0.5 * torch.sin(xx / W * 4.0)[None] + 0.4 * torch.cos(yy / H * 3.0)[None] + 0.05 * rnd(F, H, W)
    depth = depth * (1.0 + 0.3 * (torch.arange(F, device=device, dtype=dtype) % 3)).view(F, 1, 1)
    ext = torch.zeros(F, 3, 4, device=device, dtype=dtype)
    ext[:, :, :3] = torch.eye(3, device=device, dtype=dtype) + 0.01 * rnd(F, 3, 3)
    ext[:, :, 3] = 0.05 * rnd(F, 3)
    intr = torch.tensor([0.9 * W, 0.9 * W, W / 2.0, H / 2.0], device=device, dtype=dtype).repeat(F, 1)
    warp = 0.4 * rnd(F, 2, H, W)
    flows = [2.0 * rnd(P, 2, H, W) for _ in range(2)]
    weights = [torch.ones(P, H, W, device=device, dtype=dtype) for _ in range(2)]
    pf = torch.tensor(np.asarray(pairs, np.int32), device=device)
    return depth, ext, intr, warp, pf, flows[0], flows[1], weights[0], weights[1]


def device_call(solver, desc, arrays, out, grad):
    depth, ext, intr, warp, pf, fab, fba, wab, wba = arrays
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    solver._check(solver._fn("consistency_loss_device")(solver._h, C.byref(desc), p(depth), p(ext), p(intr), p(warp), p(pf), p(fab), p(fba),
                                                        p(wab), p(wba), p(out), C.c_void_p(out.data_ptr() + 8), p(grad),
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def timed(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def torch_loss(depth, ext, intr, warp, pf, fab, fba, wab, wba, lam_ratio=100.0):
    """reproj + depth ratio with the l1 distance, written from the formulas (no code of the reference): total, scalar tensor."""
    F, H, W = depth.shape
    dt, dev = depth.dtype, depth.device
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=dt), torch.arange(W, device=dev, dtype=dt), indexing="ij")
    pix = torch.stack([xx, yy], 0)[None] + warp                                    # [F, 2, H, W]
    pf = pf.long()
    total = 0.0
    for k, (flow, wgt) in enumerate(((fab, wab), (fba, wba))):
        r, t = pf[:, k], pf[:, 1 - k]
        p = pix[r]
        ray = torch.stack([(p[:, 0] - intr[r, 2, None, None]) / intr[r, 0, None, None],
                           -(p[:, 1] - intr[r, 3, None, None]) / intr[r, 1, None, None], -torch.ones_like(p[:, 0])], 1)
        Xr = (ray * depth[r][:, None]).flatten(2)                                   # [P, 3, HW]
        world = torch.baddbmm(ext[r][:, :, 3:], ext[r][:, :, :3], Xr)
        Xt = torch.bmm(ext[t][:, :, :3].transpose(1, 2), world - ext[t][:, :, 3:]).view(-1, 3, H, W)
        proj = torch.stack([intr[t, 2, None, None] + intr[t, 0, None, None] * Xt[:, 0] / -Xt[:, 2],
                            intr[t, 3, None, None] - intr[t, 1, None, None] * Xt[:, 1] / -Xt[:, 2]], 1)
        m = p + flow
        e_rep = torch.norm(proj - m, dim=1)
        size = torch.tensor([W - 1, H - 1], device=dev, dtype=dt).view(1, 2, 1, 1)
        grid = (2 * m / size - 1).permute(0, 2, 3, 1)
        zw = -torch.nn.functional.grid_sample(depth[t][:, None], grid, padding_mode="border", align_corners=False)[:, 0]
        a, b = zw.abs(), Xt[:, 2].abs()
        e_rat = lam_ratio * torch.log(torch.minimum(a, b) / torch.maximum(a, b))
        n = wgt.flatten(1).sum(1).clamp(min=1e-6)
        total = total + 0.5 * ((wgt * e_rep.abs()).flatten(1).sum(1) / n + (wgt * e_rat.abs()).flatten(1).sum(1) / n)
    return total.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=4140)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--height", type=int, default=224)
    args = ap.parse_args()
    H, W = args.height, args.width
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    solver = api.Solver(0)
    every = np.asarray(synth.hierarchical_pairs(args.frames, extra_offsets=6))   # 4140 directed pairs at 300 frames
    every = every[every[:, 0] != every[:, 1]][:args.pairs]
    problems = {"batch": (8, [(2 * b, 2 * b + 1) for b in range(4)]), "video": (args.frames, every.tolist())}
    result = {"width": W, "height": H}
    for name, (F, pairs) in problems.items():
        P, npx = len(pairs), H * W
        for dtype in (torch.float32, torch.float64):
            es = 4 if dtype == torch.float32 else 8
            arrays = make_inputs(F, pairs, H, W, dtype, dev)
            desc = api.consistency_desc(dtype == torch.float64, F, P, H, W, "l1", 1.0, 1.0, (1.0, 0.0, 100.0), True)
            out = torch.empty(1 + 3 * P, dtype=torch.float64, device=dev)
            grad = torch.empty_like(arrays[0])
            fwd = timed(lambda: device_call(solver, desc, arrays, out, None), args.calls)
            both = timed(lambda: device_call(solver, desc, arrays, out, grad), args.calls)
            bytes_fwd = P * 2 * npx * 7 * es
            bytes_both = 2 * bytes_fwd + F * npx * es + P * 2 * npx * 5 * 2 * es
            key = f"{name}_{'f32' if es == 4 else 'f64'}"
            result[key] = {"frames": F, "pairs": P, "forward_ms": fwd[0], "forward_backward_ms": both[0],
                           "forward_mb": bytes_fwd / 1e6, "forward_share_of_hbm_peak": bytes_fwd / (fwd[0] * 1e-3) / HBM_PEAK,
                           "forward_backward_mb": bytes_both / 1e6,
                           "forward_backward_share_of_hbm_peak": bytes_both / (both[0] * 1e-3) / HBM_PEAK,
                           "total": float(out[0])}
            print(f"{key}: {F} frames, {P} pairs: forward {fwd[0]:.3f} ms ({fwd[1]:.3f} .. {fwd[2]:.3f}), {bytes_fwd / 1e6:.0f} MB -> "
                  f"{100 * result[key]['forward_share_of_hbm_peak']:.1f} % of 8 TB/s; forward + backward {both[0]:.3f} ms "
                  f"({both[1]:.3f} .. {both[2]:.3f}), {bytes_both / 1e6:.0f} MB -> "
                  f"{100 * result[key]['forward_backward_share_of_hbm_peak']:.1f} %; total {float(out[0]):.6f}", flush=True)
            if name == "batch":
                depth, ext, intr, warp, pf, fab, fba, wab, wba = arrays
                B = P
                opt = types.SimpleNamespace(distance_type_static="l1", distance_scale=1.0, distance_alpha=1.0,
                                            lambda_static_reprojection=1.0, lambda_static_disparity=0.0,
                                            lambda_static_depth_ratio=100.0, recon="i3d")
                module = ConsistencyLoss(opt)
                norm = torch.tensor([W / 2, H / 2], device=dev, dtype=dtype).view(1, 2, 1, 1)
                meta = {"extrinsics": ext.view(B, 2, 3, 4), "intrinsics": intr.view(B, 2, 4), "warp": (warp / norm).view(B, 2, 2, H, W),
                        "geometry_consistency": {"flows": (fab, fba), "masks": (wab.view(B, 1, H, W), wba.view(B, 1, H, W))}}

                def module_step():
                    d = depth.view(B, 2, H, W).detach().requires_grad_(True)
                    loss, _ = module(d, meta)
                    loss.backward()
                    return loss

                def torch_step():
                    d = depth.detach().requires_grad_(True)
                    loss = torch_loss(d, ext, intr, warp, pf, fab, fba, wab, wba)
                    loss.backward()
                    return loss

                for fn, label in ((module_step, "module"), (torch_step, "plain_torch")):
                    for _ in range(3):
                        value = float(fn().detach())
                    torch.cuda.synchronize()
                    wall = []
                    for _ in range(args.calls):
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        wall.append((time.perf_counter() - t0) * 1e3)
                    result[key][f"{label}_call_backward_wall_ms"] = float(np.median(wall))
                    result[key][f"{label}_total"] = value
                    print(f"{key}: {label} call + backward, wall clock {np.median(wall):.3f} ms (median of {len(wall)}); loss {value:.6f}",
                          flush=True)
            del arrays, out, grad
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
