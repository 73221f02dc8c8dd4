"""Development aid (GPU): the scene-flow loss of flow pairs (cvd_sceneflow.h, the reference's SceneFlowLoss) through the device
entry point, in f32 and f64, at a training batch (B = 4 pairs x 6 frames of 384 x 224), l1 distances, lambdas (1, 1, 1, 100), warp
on, every mask 1 and every anchor valid (the most work a batch can ask for).
  * kernel ms of the forward pass and of forward + backward: torch events around the enqueued call (inputs resident, no copies),
    median of --calls after warm-up;
  * the backward pass's atomic additions: per pixel of a pair 2 x (1 + 4) for the static directions and 2 x (1 + 8) for the
    smooth anchors = 28 (fewer where a tap falls outside the image): additions per second, and added bytes per second (one value
    of the arrays' precision each);
  * the wall clock of one robust_cvd_amd.scene_flow.SceneFlowLoss call with .backward(), host side included;
  * the same loss written in plain torch from the formulas of DESIGN.md §3.11, forward + backward, as the device baseline.
Usage: python tools/sceneflow_bench.py [--calls 20] [--batch 4]"""
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

from robust_cvd_amd import api
from robust_cvd_amd.scene_flow import SceneFlowLoss

LAMBDAS = (1.0, 1.0, 1.0, 100.0)


def make_inputs(B, H, W, dtype, device, seed=3):
    """The module's layout: F = 6 B frames, frame 6 b + k = (ref, target, ref - 1, ref + 1, target - 1, target + 1)."""
    g = torch.Generator(device=device).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, device=device, dtype=dtype)
    F = 6 * B
    yy, xx = torch.meshgrid(torch.arange(H, device=device, dtype=dtype), torch.arange(W, device=device, dtype=dtype), indexing="ij")
    depth = 3.0 + 0.5 * torch.sin(xx / W * 4.0)[None] + 0.4 * torch.cos(yy / H * 3.0)[None] + 0.05 * rnd(F, H, W)
    depth = depth * (1.0 + 0.3 * (torch.arange(F, device=device, dtype=dtype) % 3)).view(F, 1, 1)
    ext = torch.zeros(F, 3, 4, device=device, dtype=dtype)
    ext[:, :, :3] = torch.eye(3, device=device, dtype=dtype) + 0.01 * rnd(F, 3, 3)
    ext[:, :, 3] = 0.05 * rnd(F, 3)
    intr = torch.tensor([0.9 * W, 0.9 * W, W / 2.0, H / 2.0], device=device, dtype=dtype).repeat(F, 1)
    warp = 0.4 * rnd(F, 2, H, W)
    flows = [2.0 * rnd(B, 2, H, W) for _ in range(2)]
    masks = [torch.ones(B, H, W, device=device, dtype=dtype) for _ in range(2)]
    nflows = [2.0 * rnd(B, 2, H, W) for _ in range(4)]
    nmasks = [torch.ones(B, H, W, device=device, dtype=dtype) for _ in range(4)]
    valid = torch.ones(B, 2, device=device, dtype=dtype)
    base = torch.arange(B, dtype=torch.int32, device=device).view(B, 1) * 6
    pairs = (base + torch.arange(2, dtype=torch.int32, device=device).view(1, 2)).contiguous()
    nbrs = (base + torch.arange(2, 6, dtype=torch.int32, device=device).view(1, 4)).contiguous()
    return dict(depth=depth, ext=ext, intr=intr, warp=warp, pairs=pairs, flows=flows, masks=masks, nbrs=nbrs, nflows=nflows,
                nmasks=nmasks, valid=valid)


def device_call(solver, desc, a, out, grad):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    group = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    solver._check(solver._fn("scene_flow_loss_device")(
        solver._h, C.byref(desc), p(a["depth"]), p(a["ext"]), p(a["intr"]), p(a["warp"]), p(a["pairs"]), group(a["flows"]),
        group(a["masks"]), p(a["nbrs"]), group(a["nflows"]), group(a["nmasks"]), p(a["valid"]), p(out),
        C.c_void_p(out.data_ptr() + 8), p(grad), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))


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


def torch_loss(a, depth, lam=LAMBDAS):
    """All four terms with the l1 distance, written from the formulas (no code of the reference): total, scalar tensor."""
    F, H, W = depth.shape
    dt, dev = depth.dtype, depth.device
    ext, intr = a["ext"], a["intr"]
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=dt), torch.arange(W, device=dev, dtype=dt), indexing="ij")
    pix = torch.stack([xx, yy], 0)[None] + a["warp"]                                                   # [F, 2, H, W]
    ray = torch.stack([(pix[:, 0] - intr[:, 2, None, None]) / intr[:, 0, None, None],
                       -(pix[:, 1] - intr[:, 3, None, None]) / intr[:, 1, None, None], -torch.ones_like(pix[:, 0])], 1)
    X = ray * depth[:, None]                                                                            # [F, 3, H, W]
    size = torch.tensor([W - 1, H - 1], device=dev, dtype=dt).view(1, 2, 1, 1)
    R, t = ext[:, :, :3], ext[:, :, 3:]

    def world(f, pts):
        return torch.baddbmm(t[f], R[f], pts.flatten(2)).view(-1, 3, H, W)

    def matched(f, m):      # R_f S_f(m) + t_f
        grid = (2 * m / size - 1).permute(0, 2, 3, 1)
        return world(f, torch.nn.functional.grid_sample(X[f], grid, padding_mode="border", align_corners=False))

    def term(rho, w):
        return (w * rho).flatten(1).sum(1) / w.flatten(1).sum(1).clamp(min=1e-6)

    pairs, nbrs = a["pairs"].long(), a["nbrs"].long()
    total = 0.0
    for k in range(2):
        r, tg = pairs[:, k], pairs[:, 1 - k]
        d = torch.norm(world(r, X[r]) - matched(tg, pix[r] + a["flows"][k]), dim=1)
        total = total + 0.5 * lam[0] * term(d, a["masks"][k] / depth[r].abs())
        n0, n1 = nbrs[:, 2 * k], nbrs[:, 2 * k + 1]
        Xw = world(r, X[r])
        Q = matched(n1, pix[r] + a["nflows"][2 * k + 1]) + matched(n0, pix[r] + a["nflows"][2 * k]) - Xw - t[r][:, :, :, None]
        Xs = torch.bmm(R[r].transpose(1, 2), Q.flatten(2)).view(-1, 3, H, W)
        w = a["valid"][:, k, None, None] * a["nmasks"][2 * k] * a["nmasks"][2 * k + 1]
        proj = torch.stack([intr[r, 2, None, None] + intr[r, 0, None, None] * Xs[:, 0] / -Xs[:, 2],
                            intr[r, 3, None, None] - intr[r, 1, None, None] * Xs[:, 1] / -Xs[:, 2]], 1)
        e_rep = torch.norm(proj - pix[r], dim=1)
        e_dsp = 1.0 / Xs[:, 2] - 1.0 / X[r][:, 2]
        p, q = X[r][:, 2].abs(), Xs[:, 2].abs()
        e_rat = lam[3] * torch.log(torch.minimum(p, q) / torch.maximum(p, q))
        fbar = intr[r, :2].mean()
        total = total + 0.5 * (lam[1] * term(e_rep, w) + lam[2] * fbar * term(e_dsp.abs(), w) + term(e_rat.abs(), w))
    return total.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--height", type=int, default=224)
    args = ap.parse_args()
    H, W, B = args.height, args.width, args.batch
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    solver = api.Solver(0)
    result = {"width": W, "height": H, "pairs": B, "frames": 6 * B}
    npx = H * W
    for dtype in (torch.float32, torch.float64):
        es = 4 if dtype == torch.float32 else 8
        a = make_inputs(B, H, W, dtype, dev)
        desc = api.scene_flow_desc(dtype == torch.float64, 6 * B, B, H, W, "l1", "l1", 1.0, 1.0, LAMBDAS, True)
        out = torch.empty(1 + 4 * B, dtype=torch.float64, device=dev)
        grad = torch.empty_like(a["depth"])
        fwd = timed(lambda: device_call(solver, desc, a, out, None), args.calls)
        both = timed(lambda: device_call(solver, desc, a, out, grad), args.calls)
        adds = B * npx * 28
        back_ms = both[0] - fwd[0]
        key = "f32" if es == 4 else "f64"
        result[key] = {"forward_ms": fwd[0], "forward_backward_ms": both[0], "backward_ms": back_ms, "atomic_adds": adds,
                       "adds_per_s": adds / (back_ms * 1e-3), "added_bytes_per_s": adds * es / (back_ms * 1e-3),
                       "total": float(out[0])}
        print(f"{key}: {B} pairs, {6 * B} frames of {W} x {H}: forward {fwd[0]:.3f} ms ({fwd[1]:.3f} .. {fwd[2]:.3f}); forward + "
              f"backward {both[0]:.3f} ms ({both[1]:.3f} .. {both[2]:.3f}); backward {back_ms:.3f} ms for {adds / 1e6:.1f} M adds -> "
              f"{adds / (back_ms * 1e-3) / 1e9:.1f} G adds/s, {adds * es / (back_ms * 1e-3) / 1e9:.1f} GB/s added; total {float(out[0]):.6f}",
              flush=True)
        opt = types.SimpleNamespace(distance_type_static="l1", distance_type_smooth="l1", distance_scale=1.0, distance_alpha=1.0,
                                    lambda_scene_flow_static=LAMBDAS[0], lambda_smooth_reprojection=LAMBDAS[1],
                                    lambda_smooth_disparity=LAMBDAS[2], lambda_smooth_depth_ratio=LAMBDAS[3], recon="i3d")
        module = SceneFlowLoss(opt)
        norm = torch.tensor([W / 2, H / 2], device=dev, dtype=dtype).view(1, 2, 1, 1)
        meta = {"extrinsics": a["ext"].view(B, 6, 3, 4), "intrinsics": a["intr"].view(B, 6, 4),
                "warp": (a["warp"] / norm).view(B, 6, 2, H, W),
                "geometry_consistency": {"flows": tuple(a["flows"]), "masks": tuple(m.view(B, 1, H, W) for m in a["masks"])},
                "temporal_smoothness": {"flows": tuple(a["nflows"]), "masks": tuple(m.view(B, 1, H, W) for m in a["nmasks"]),
                                        "valid": a["valid"].view(B, 2, 1)}}

        def module_step():
            d = a["depth"].view(B, 6, H, W).detach().requires_grad_(True)
            loss, _, _ = module(d, meta)
            loss.backward()
            return loss

        def torch_step():
            d = a["depth"].detach().requires_grad_(True)
            loss = torch_loss(a, d)
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
        del a, out, grad
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
