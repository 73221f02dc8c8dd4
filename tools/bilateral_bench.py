"""Development aid (GPU): the bilateral depth filter (cvd_bilateral.h, DepthVideoProcessor::bilateralFilter) at the benchmark's
size (300 frames, 384 x 224).  Kernel times come from HIP events around the launches (host<->device copies excluded); GB/s =
algorithmic bytes / kernel time, counting per output pixel every input frame of its window once (depth 4 B, + BGR colour
12 B when the colour term is on) and 4 B written.  The in-place default is timed as the whole drop-in op (wall clock: one
call per frame, files, host transform).  The CPU figure is the numpy restatement (tests/bilateral_reference.py), for context.
Usage: python tools/bilateral_bench.py"""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from robust_cvd_amd import api, dataset_io, synth
from tests.bilateral_reference import bilateral_filter

F, W, H = 300, 384, 224
rng = np.random.default_rng(0)
depth = rng.uniform(1.0, 3.0, (F, H, W)).astype(np.float32)
color = rng.uniform(0.0, 1.0, (F, H, W, 3)).astype(np.float32)
s = api.Solver(0)
px = F * W * H

cases = (("default (R 2, r 0, depthSigma 0.3), out of place", dict(frame_radius=2), 0),
         ("R 2, r 2, colorSigma 0.1", dict(frame_radius=2, spatial_radius=2, color_sigma=0.1), 1),
         ("median, R 2, r 3", dict(frame_radius=2, spatial_radius=3, median=True), 0))
for name, kw, use_color in cases:
    c = color if use_color else None
    s.bilateral_filter(depth[:6], c[:6] if use_color else None, **kw)   # warm-up
    times = []
    for _ in range(5):
        out, ms = s.bilateral_filter(depth, c, timing=True, **kw)
        times.append(ms)
    ms = float(np.median(times))
    R = kw["frame_radius"]
    frames_read = sum(min(F - 1, f + R) - max(0, f - R) + 1 for f in range(F))
    alg = frames_read * W * H * (4 + 12 * use_color) + px * 4
    m = 2
    t0 = time.perf_counter()
    bilateral_filter(depth[:R + m], color[:R + m], count=m, **kw) if not kw.get("median") else \
        bilateral_filter(depth[:R + 1, :24, :48], color[:R + 1, :24, :48], count=1, **kw)
    dc = time.perf_counter() - t0
    cpu = dc / m if not kw.get("median") else dc * (W * H) / (24 * 48)
    print(f"{name}: {F} frames in {ms:.3f} ms kernel time (median of 5: {', '.join(f'{t:.3f}' for t in times)}); "
          f"algorithmic {alg / 1e6:.0f} MB -> {alg / ms / 1e6:.0f} GB/s; CPU restatement (numpy) {cpu * 1e3:.0f} ms per frame")

# in place, the drop-in module's default call (depthStream 0), whole op
from robust_cvd_amd import build as b
sys.path.insert(0, os.path.dirname(b.build_lib_python()))
import lib_python as lib

with tempfile.TemporaryDirectory() as tmp:
    v = synth.make_video(F, W, H, seed=1)
    base = dataset_io.write_dataset(os.path.join(tmp, "v"), v)
    dataset_io.write_flow_inputs(base, [], [], [], color)
    dv = lib.DepthVideo()
    lib.DepthVideoImporter.importVideo(dv, base, True)
    dv.createDepthStream("depth", "depth", [W, H])
    ds = dv.depthStream(0)
    for f in range(F):
        ds.frame(f).setDepth(depth[f])
    proc = lib.DepthVideoProcessor(dv)
    p = lib.DepthVideoProcessor.Params()
    p.op = lib.DepthVideoProcessor.Op.BilateralFilter
    p.frameRange.fromString(f"0-{F - 1}")
    t0 = time.perf_counter()
    proc.process(p)
    dt = time.perf_counter() - t0
    print(f"in place default (drop-in Op.BilateralFilter, depthStream 0): {F} frames in {dt:.2f} s wall clock "
          f"({dt / F * 1e3:.1f} ms per frame: one call each, colour files read, host transform)")
