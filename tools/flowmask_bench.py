"""Development aid (GPU): the flow consistency masks (cvd_flowmask.h, Flow.compute_flow_masks) at the benchmark's size: 300
colour frames of 384 x 224 and 256 unordered pairs of the hierarchical pair list (both directions each: 512 masks).
Kernel times come from HIP events around the launch (copies excluded), over 20 timed calls per thread-to-pixel map after
warm-up, the two maps alternating.  Algorithmic bytes = both flows + both masks per pair and the colour table once; the 256
pairs hold 352 MB of flow, past the 256 MiB Infinity Cache, so bytes / time is compared with the HBM peak (8 TB/s).  The
per-call time is the wall clock of Solver.flow_consistency_masks (host-to-device copies of colours and flows, the kernel, the
copy of the masks back).  The file-level figure is compute_flow_masks on a dataset directory (reads, calls, PNG writes); the
CPU figure is the numpy restatement (tests/flowmask_reference.py) on 8 of the pairs.
Usage: python tools/flowmask_bench.py [--pairs 256] [--frames 300] [--calls 20]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from robust_cvd_amd import api, dataset_io, flow_masks, synth
from tests import flowmask_cases as fc
from tests import flowmask_reference as fr

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=256)
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--width", type=int, default=384)
ap.add_argument("--height", type=int, default=224)
args = ap.parse_args()
F, W, H, P, C = args.frames, args.width, args.height, args.pairs, 3

s = api.Solver(0)  # (first: a machine without a GPU fails here, before any set-up work)
t0 = time.perf_counter()
every = synth.hierarchical_pairs(F)
un = np.array([p for p in np.asarray(every).tolist() if p[0] < p[1]], np.int32)
un = un[np.linspace(0, len(un) - 1, P).astype(np.int64)]          # P unordered pairs spread over the video and the levels
directed = np.concatenate([un, un[:, ::-1]])
directed = directed[np.lexsort((directed[:, 1], directed[:, 0]))]
video = synth.make_video(F, W, H, seed=1, pairs=directed, spacing=50.0)
flow, _mask = synth.make_dense_flows(video, flow_noise_px=0.35, seed=5, invalid_fraction=0)
pairs, iab, iba = fc.unordered_pairs(video)
flow_ab, flow_ba = np.ascontiguousarray(flow[iab]), np.ascontiguousarray(flow[iba])
del flow
color = fc.colors(F, W, H, C)
npx = W * H
print(f"inputs: {F} frames {W} x {H}, {len(pairs)} pairs ({flow_ab.nbytes * 2 / 1e6:.0f} MB of flow, {color.nbytes / 1e6:.0f} MB of "
      f"colour), built in {time.perf_counter() - t0:.1f} s", flush=True)

run = lambda pix, **kw: s.flow_consistency_masks(color, pairs, flow_ab, flow_ba, 1.0, 1.0, pixels_per_thread=pix, **kw)
ref = None
for pix in (1, 4, 1, 4):                                            # warm-up: both maps, twice
    out = run(pix)
    ref = ref or out
    assert out[0].tobytes() == ref[0].tobytes() and out[1].tobytes() == ref[1].tobytes() and np.array_equal(out[2], ref[2])
kernel, call = {1: [], 4: []}, {1: [], 4: []}
for _ in range(args.calls):
    for pix in (1, 4):
        t0 = time.perf_counter()
        out = run(pix, timing=True)
        call[pix].append((time.perf_counter() - t0) * 1e3)
        kernel[pix].append(out[-1])
alg = len(pairs) * (2 * npx * 8 + 2 * npx) + F * npx * C * 4
result = {"frames": F, "width": W, "height": H, "pairs": int(len(pairs)), "algorithmic_mb": alg / 1e6,
          "kept_share": float(ref[2].sum() / (2 * len(pairs) * npx))}
for pix in (1, 4):
    k, c = np.array(kernel[pix]), np.array(call[pix])
    result[f"pix{pix}"] = {"kernel_ms_median": float(np.median(k)), "kernel_ms_min": float(k.min()), "kernel_ms_max": float(k.max()),
                           "call_ms_median": float(np.median(c)), "tb_per_s": alg / np.median(k) / 1e9,
                           "share_of_8tbs": alg / np.median(k) / 1e9 / 8.0}
    print(f"{pix} pixel(s) per thread: kernel {np.median(k):.3f} ms (median of {len(k)}, {k.min():.3f} .. {k.max():.3f}); algorithmic "
          f"{alg / 1e6:.0f} MB -> {alg / np.median(k) / 1e9:.2f} TB/s = {100 * alg / np.median(k) / 1e9 / 8.0:.1f} % of 8 TB/s; call with "
          f"copies {np.median(c):.1f} ms ({np.median(c) / len(pairs):.3f} ms per pair)", flush=True)

n = min(8, len(pairs))
t0 = time.perf_counter()
rab, rba, _k, _e = fr.batch(color, pairs[:n], flow_ab[:n], flow_ba[:n], 1.0, 1.0)
cpu = (time.perf_counter() - t0) / n
differ = int((rab != ref[0][:n]).sum() + (rba != ref[1][:n]).sum())
result["numpy_ms_per_pair"] = cpu * 1e3
print(f"numpy restatement (f64): {cpu * 1e3:.1f} ms per pair -> {cpu * len(pairs):.1f} s for {len(pairs)} pairs; its masks differ from "
      f"the kernel's on {differ} of {2 * n * npx} pixels (f32 against f64 at the thresholds)", flush=True)

with tempfile.TemporaryDirectory() as tmp:
    t0 = time.perf_counter()
    both = np.concatenate([pairs, pairs[:, ::-1]])
    dataset_io.write_flow_inputs(tmp, both[:0], [], [], color)
    os.makedirs(os.path.join(tmp, "flow"), exist_ok=True)
    for (a, b), fl in zip(both.tolist(), list(flow_ab) + list(flow_ba)):
        dataset_io.write_raw_image(os.path.join(tmp, "flow", f"flow_{a:06d}_{b:06d}.raw"), fl)
    tw = time.perf_counter() - t0
    t0 = time.perf_counter()
    written = flow_masks.compute_flow_masks(tmp)
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    for (a, b) in both.tolist():
        dataset_io.read_raw_image(os.path.join(tmp, "flow", f"flow_{a:06d}_{b:06d}.raw"))
    for f in sorted(set(both.ravel().tolist())):
        dataset_io.read_raw_image(os.path.join(tmp, "color_down", f"frame_{f:06d}.raw"))
    tr = time.perf_counter() - t0
    from PIL import Image
    t0 = time.perf_counter()
    for i in range(len(pairs)):
        Image.fromarray(ref[0][i], "L").save(os.path.join(tmp, "probe.png"), compress_level=1)
        Image.fromarray(ref[1][i], "L").save(os.path.join(tmp, "probe.png"), compress_level=1)
    tp = time.perf_counter() - t0
    result["files"] = {"masks_written": written, "compute_flow_masks_s": dt, "reading_the_raw_files_s": tr, "png_writes_s": tp,
                       "dataset_write_s": tw}
    print(f"compute_flow_masks on files: {written} masks in {dt:.2f} s ({dt / len(pairs) * 1e3:.1f} ms per pair); of which reading the raw "
          f"files alone takes {tr:.2f} s (page cache warm) and encoding the PNGs {tp:.2f} s", flush=True)
print(json.dumps(result))
