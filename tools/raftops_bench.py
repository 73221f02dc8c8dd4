"""Development aid (GPU): RAFT's correlation pyramid, lookup and convex upsampling (csrc/cvd_raftops.h, robust_cvd_amd.raft_ops)
at the flow stage's working size: B = 1, 72 x 128 features (a 1024 x 576 input), dim 256, 4 levels, radius 4 -- an all-pairs volume
of 340 MB, past the 256 MiB Infinity Cache.

Times are HIP-event times on torch's current stream (median of --calls after warm-up).  Per kernel: the bytes it must move,
computed from the shapes (pyramid: the volume once in, the four levels out; lookup: the four (2r+2)^2 footprints of every query,
the coordinates and the output; upsampling: logits and flow in, the 8x flow out) and the share of the 8 TB/s HBM peak they imply
(the lookup's footprints are scattered 40-byte row segments: its bytes are a lower bound of its traffic, not a roofline).  The
end-to-end figure is one pair's refinement loop as far as these operators go: 20 x (lookup + upsampling) through the module,
beside the same operations written with plain torch ops (grid_sample, softmax, unfold) on the same GPU, rounds alternating; the
two agree within the suite's bars (checked here on the first call).  Seeded random inputs (never zeros).
Usage: python tools/raftops_bench.py [--out profiles/raftops_bench.json] [--calls 20] [--h 72 --w 128 --dim 256]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from robust_cvd_amd.raft_ops import CorrBlock, upsample_flow

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--h", type=int, default=72)
ap.add_argument("--w", type=int, default=128)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--levels", type=int, default=4)
ap.add_argument("--radius", type=int, default=4)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("raftops_bench needs a GPU: there is nothing to measure without one")
dev = torch.device("cuda", 0)
B, h, w, dim, L, r = 1, args.h, args.w, args.dim, args.levels, args.radius
n = 2 * r + 1
Q = B * h * w
PEAK = 8.0e12


def torch_pyramid(raw):
    """The pyramid with stock ops: one division and L - 1 poolings."""
    levels = [raw.view(Q, 1, h, w) / torch.sqrt(torch.tensor(float(dim)))]
    for _ in range(L - 1):
        levels.append(F.avg_pool2d(levels[-1], 2, stride=2))
    return levels


def torch_lookup(levels, coords):
    """The lookup with stock ops: per level a window of sampling positions around every query, grid_sample on [Q, 1, h_l, w_l]."""
    centre = coords.permute(0, 2, 3, 1).reshape(Q, 1, 1, 2)
    d = torch.linspace(-r, r, n, device=coords.device)
    window = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1).view(1, n, n, 2)     # [a, b] -> (d[a], d[b]): a moves x
    out = []
    for l, vol in enumerate(levels):
        pos = centre / 2 ** l + window
        hl, wl = vol.shape[-2:]
        grid = torch.stack([2 * pos[..., 0] / (wl - 1) - 1, 2 * pos[..., 1] / (hl - 1) - 1], dim=-1)
        out.append(F.grid_sample(vol, grid, align_corners=True).view(B, h, w, n * n))
    return torch.cat(out, dim=-1).permute(0, 3, 1, 2).contiguous().float()


def torch_upsample(flow, mask):
    """The convex upsampling with stock ops: softmax over the nine logits, unfold, product, sum, permute."""
    N, _, H, W = flow.shape
    p = torch.softmax(mask.view(N, 1, 9, 8, 8, H, W), dim=2)
    nb = F.unfold(8 * flow, [3, 3], padding=1).view(N, 2, 9, 1, 1, H, W)
    return torch.sum(p * nb, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * H, 8 * W)


def event_ms(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    t = np.array(times)
    return {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max()), "calls": calls}


def with_rate(stat, nbytes):
    stat = dict(stat, bytes=int(nbytes))
    stat["tb_per_s"] = nbytes / (stat["ms_median"] * 1e-3) / 1e12
    stat["share_of_8tbs"] = nbytes / (stat["ms_median"] * 1e-3) / PEAK
    return stat


torch.manual_seed(20260)
with torch.no_grad():
    fmap1 = torch.randn(B, dim, h, w, device=dev)
    fmap2 = torch.randn(B, dim, h, w, device=dev)
    gy, gx = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    coords = torch.stack([gx, gy])[None] + 6.0 * torch.randn(B, 2, h, w, device=dev)
    flow = 3.0 * torch.randn(B, 2, h, w, device=dev)
    mask = 2.0 * torch.randn(B, 576, h, w, device=dev)
    raw = torch.matmul(fmap1.view(B, dim, h * w).transpose(1, 2), fmap2.view(B, dim, h * w))

    block = CorrBlock(fmap1, fmap2, num_levels=L, radius=r)
    ref_levels = torch_pyramid(raw)
    level_cells = [t.shape[-2] * t.shape[-1] for t in block.corr_pyramid]
    checks = {"level0_equal": bool(torch.equal(block.corr_pyramid[0], ref_levels[0])),
              "pooled_max_abs_diff": max(float((a - b).abs().max()) for a, b in zip(block.corr_pyramid[1:], ref_levels[1:])),
              "lookup_max_abs_diff": float((block(coords) - torch_lookup(ref_levels, coords)).abs().max()),
              "upsample_max_abs_diff": float((upsample_flow(flow, mask) - torch_upsample(flow, mask)).abs().max())}
    print("module against the torch baseline:", checks, flush=True)
    # (gross agreement only: the bars are the suite's; level 0 is equal when torch's two matmul calls give the same bits)
    assert checks["pooled_max_abs_diff"] < 1e-3 and checks["lookup_max_abs_diff"] < 1e-2 and checks["upsample_max_abs_diff"] < 1e-2, checks

    result = {"shape": {"B": B, "h": h, "w": w, "dim": dim, "levels": L, "radius": r, "volume_mb": Q * h * w * 4 / 1e6},
              "checks": checks}
    # the pyramid kernel alone (in place on a scratch copy of the product: the division is repeated, the bytes are the same)
    scratch = raw.clone()
    table = block._table.__class__(*([scratch.data_ptr()] + [t.data_ptr() for t in block.corr_pyramid[1:]]))
    from robust_cvd_amd import raft_ops as _ro
    import ctypes as C
    pyr_call = lambda: _ro._call(dev, "raft_corr_pyramid_device", C.c_int64(Q), C.c_int32(h), C.c_int32(w), C.c_int32(dim), C.c_int32(L),
                                 C.c_void_p(scratch.data_ptr()), table)
    pyr_bytes = 4 * Q * (h * w + sum(level_cells))
    result["pyramid"] = with_rate(event_ms(pyr_call, args.calls), pyr_bytes)
    result["pyramid_torch"] = event_ms(lambda: torch_pyramid(raw), args.calls)
    block = CorrBlock(fmap1, fmap2, num_levels=L, radius=r)        # (the timed launches rescaled level 0 of the old pyramid's copy only)
    look_bytes = 4 * Q * (L * (2 * r + 2) ** 2 + 2 + L * n * n)
    result["lookup"] = with_rate(event_ms(lambda: block(coords), args.calls), look_bytes)
    result["lookup_torch"] = event_ms(lambda: torch_lookup(ref_levels, coords), args.calls)
    up_bytes = 4 * B * h * w * (576 + 2 + 2 * 64)
    result["upsample"] = with_rate(event_ms(lambda: upsample_flow(flow, mask), args.calls), up_bytes)
    result["upsample_torch"] = event_ms(lambda: torch_upsample(flow, mask), args.calls)

    def loop_module():
        for _ in range(args.iters):
            block(coords)
            upsample_flow(flow, mask)

    def loop_torch():
        for _ in range(args.iters):
            torch_lookup(ref_levels, coords)
            torch_upsample(flow, mask)

    rounds = {"module": [], "torch": []}
    for _ in range(max(args.calls // 4, 3)):                       # alternating rounds in one process
        rounds["module"].append(event_ms(loop_module, 1, warmup=1)["ms_median"])
        rounds["torch"].append(event_ms(loop_torch, 1, warmup=1)["ms_median"])
    result["loop"] = {"iterations": args.iters,
                      "module_ms_median": float(np.median(rounds["module"])), "module_ms_min": float(np.min(rounds["module"])),
                      "torch_ms_median": float(np.median(rounds["torch"])), "torch_ms_min": float(np.min(rounds["torch"])),
                      "rounds": len(rounds["module"])}
    result["loop"]["speedup"] = result["loop"]["torch_ms_median"] / result["loop"]["module_ms_median"]

for key in ("pyramid", "lookup", "upsample"):
    k, t = result[key], result[key + "_torch"]
    print(f"{key}: kernel {k['ms_median']:.3f} ms (median of {k['calls']}, {k['ms_min']:.3f} .. {k['ms_max']:.3f}); {k['bytes'] / 1e6:.1f} MB "
          f"-> {k['tb_per_s']:.2f} TB/s = {100 * k['share_of_8tbs']:.1f} % of 8 TB/s; torch ops {t['ms_median']:.3f} ms", flush=True)
lp = result["loop"]
print(f"{lp['iterations']} x (lookup + upsampling): module {lp['module_ms_median']:.2f} ms, torch ops {lp['torch_ms_median']:.2f} ms "
      f"(x {lp['speedup']:.2f}; medians of {lp['rounds']} alternating rounds)", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
print(json.dumps(result))
