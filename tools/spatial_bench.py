"""Development aid (GPU): the spatial smoothness and contrast losses (cvd_spatial.h, the reference's DisparitySmoothLoss and
ContrastLoss) through the device entry point, both terms on, in f32 and f64, at 8 and at 300 frames of 384 x 224 (samples of two
frames).
  * kernel ms of the pass with and without the gradient: torch events around the enqueued call (inputs resident, no copies),
    median of --calls after warm-up;
  * algorithmic bytes: per pixel five values read (depth, original depth, three colours) and, with the gradient, one written;
    their rate and its share of the 8 TB/s of the device's memory;
  * the wall clock of one robust_cvd_amd.spatial_losses.spatial_terms call with .backward(), host side included;
  * the same two terms written in plain torch from the formulas of DESIGN.md §3.12, forward + backward, as the device baseline.
Usage: python tools/spatial_bench.py [--calls 20] [--frames 8 300]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # (before the library is loaded: the process then holds one HIP runtime)

from robust_cvd_amd import api
from robust_cvd_amd.spatial_losses import spatial_terms

SETTINGS = dict(lambda_disparity_smooth=0.5, sigma_color_grad=1.0, lambda_contrast_loss=1.0, contrast_thresh=1.05)
PEAK_BYTES_PER_S = 8e12
N = 2


def make_inputs(F, H, W, dtype, device, seed=3):
    g = torch.Generator(device=device).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=device), torch.arange(W, device=device), indexing="ij")
    steps = 1.3 ** torch.randint(0, 4, (F, (H + 2) // 3, (W + 2) // 3), generator=g, device=device).to(dtype)[:, yy // 3, xx // 3]
    base = 2.0 + 0.1 * torch.sin(xx.to(dtype) / W * 2.0)[None] + 0.1 * torch.cos(yy.to(dtype) / H * 2.0)[None]
    noise = lambda: 1.0 + 0.01 * torch.randn(F, H, W, generator=g, device=device, dtype=dtype)
    orig = base * steps * noise()
    depth = base * steps * noise() * 1.02
    image = torch.rand(F, 3, H, W, generator=g, device=device, dtype=dtype)
    return depth.contiguous(), orig.contiguous(), image.contiguous()


def device_call(solver, desc, depth, orig, image, out, grad):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    solver._check(solver._fn("spatial_losses_device")(
        solver._h, C.byref(desc), p(depth), p(orig), p(image), p(out), C.c_void_p(out.data_ptr() + 16),
        C.c_void_p(out.data_ptr() + 8), p(grad), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


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


def torch_loss(depth, orig, image, lambda_disparity_smooth, sigma_color_grad, lambda_contrast_loss, contrast_thresh):
    """Both terms written from the formulas (no code of the reference): total, scalar tensor.  depth, orig [F, H, W], image
    [F, 3, H, W]; samples of N frames."""
    F, H, W = depth.shape
    B = F // N
    d = 1.0 / depth
    sx = torch.exp(-(image[..., :, :-1] - image[..., :, 1:]).abs().mean(1) / sigma_color_grad) * (d[:, :, :-1] - d[:, :, 1:]).abs()
    sy = torch.exp(-(image[..., :-1, :] - image[..., 1:, :]).abs().mean(1) / sigma_color_grad) * (d[:, :-1, :] - d[:, 1:, :]).abs()
    smooth = lambda_disparity_smooth * (sx.reshape(B, -1).mean(1) + sy.reshape(B, -1).mean(1))
    ratio = lambda a, b: torch.maximum(a, b) / (torch.minimum(a, b) + 1e-10)
    c = 0.0
    for sl_a, sl_b in (((slice(None), slice(None), slice(0, -1)), (slice(None), slice(None), slice(1, None))),
                       ((slice(None), slice(0, -1), slice(None)), (slice(None), slice(1, None), slice(None)))):
        mask = ratio(orig[sl_a], orig[sl_b]) > contrast_thresh
        c = c + ((contrast_thresh - ratio(depth[sl_a], depth[sl_b])) ** 2 * mask).sum()
    return smooth.mean() + lambda_contrast_loss * c / F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 300])
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--height", type=int, default=224)
    args = ap.parse_args()
    H, W = args.height, args.width
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    solver = api.Solver(0)
    result = {"width": W, "height": H, "frames_per_sample": N, "runs": []}
    for F in args.frames:
        for dtype in (torch.float32, torch.float64):
            es = 4 if dtype == torch.float32 else 8
            key = "f32" if es == 4 else "f64"
            depth, orig, image = make_inputs(F, H, W, dtype, dev)
            desc = api.spatial_desc(dtype == torch.float64, F, N, H, W, **SETTINGS)
            out = torch.empty(2 + F // N, dtype=torch.float64, device=dev)
            grad = torch.empty_like(depth)
            value = timed(lambda: device_call(solver, desc, depth, orig, image, out, None), args.calls)
            both = timed(lambda: device_call(solver, desc, depth, orig, image, out, grad), args.calls)
            px = F * H * W
            read, written = 5 * px * es, px * es
            run = {"frames": F, "precision": key, "value_ms": value[0], "value_gradient_ms": both[0], "bytes_read": read,
                   "bytes_written": written, "value_bytes_per_s": read / (value[0] * 1e-3),
                   "value_gradient_bytes_per_s": (read + written) / (both[0] * 1e-3), "total": float(out[0])}
            run["value_share_of_peak"] = run["value_bytes_per_s"] / PEAK_BYTES_PER_S
            run["value_gradient_share_of_peak"] = run["value_gradient_bytes_per_s"] / PEAK_BYTES_PER_S
            print(f"{key}: {F} frames of {W} x {H}: value {value[0]:.4f} ms ({value[1]:.4f} .. {value[2]:.4f}), "
                  f"{run['value_bytes_per_s'] / 1e9:.0f} GB/s = {100 * run['value_share_of_peak']:.1f} % of 8 TB/s; value + gradient "
                  f"{both[0]:.4f} ms ({both[1]:.4f} .. {both[2]:.4f}), {run['value_gradient_bytes_per_s'] / 1e9:.0f} GB/s = "
                  f"{100 * run['value_gradient_share_of_peak']:.1f} %; total {float(out[0]):.6f}", flush=True)

            def module_step():
                d = depth.view(F // N, N, H, W).detach().requires_grad_(True)
                loss, _, _ = spatial_terms(d, orig.view(F // N, N, H, W), image.view(F // N, N, 3, H, W), **SETTINGS)
                loss.backward()
                return loss

            def torch_step():
                d = depth.detach().requires_grad_(True)
                loss = torch_loss(d, orig, image, **SETTINGS)
                loss.backward()
                return loss

            for fn, label in ((module_step, "module"), (torch_step, "plain_torch")):
                for _ in range(3):
                    v = float(fn().detach())
                torch.cuda.synchronize()
                wall = []
                for _ in range(args.calls):
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    wall.append((time.perf_counter() - t0) * 1e3)
                run[f"{label}_call_backward_wall_ms"] = float(np.median(wall))
                run[f"{label}_total"] = v
                print(f"{key}: {label} call + backward, wall clock {np.median(wall):.3f} ms (median of {len(wall)}); loss {v:.6f}",
                      flush=True)
            result["runs"].append(run)
            del depth, orig, image, out, grad
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
