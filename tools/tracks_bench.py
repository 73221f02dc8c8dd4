"""Development aid (GPU): feature tracks (cvd_tracks.h, DepthVideoProcessor::computeTracks) at 300 frames of 384 x 224 with
the default parameters (spawn 20, prune 5, min length 4) on a synth.make_video scene (flows of the true geometry, noise
colour images).  Kernel ms per phase {candidates, sort, walk, table} from HIP events and the call's wall clock (copies
included), median of 5 calls; the drop-in op DepthVideoProcessor.computeTracks on the same video written to a temporary
dataset (file reading, corner response and distance transform included); the numpy restatement tests/tracks_reference.py on
the same arrays, whose result must equal the GPU's.  Usage: python tools/tracks_bench.py [--frames N] [--no-drop-in]"""
import argparse
import importlib
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from robust_cvd_amd import api, dataset_io, synth
from robust_cvd_amd import build as _b
from tests.tracks_reference import compute_tracks, from_arrays

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--no-drop-in", action="store_true")
args = ap.parse_args()
F, W, H = args.frames, 384, 224
pairs = np.array([(f, f + 1) for f in range(F - 1)], np.int32)
v = synth.make_video(F, W, H, seed=1234, pairs=pairs)
flow, mask = synth.make_dense_flows(v, seed=5)
colors = np.random.default_rng(6).uniform(0, 1, (F, H, W, 3)).astype(np.float32)
s = api.Solver(0)
corner = s.corner_min_eigenval(colors)
active, present = np.ones(F, np.uint8), np.full(F - 1, 3, np.uint8)
call = (corner, v.inv_aspect, active, 0, F - 1, flow, mask, present, None)
s.compute_tracks(*call)   # warm-up
runs = []
for _ in range(5):
    t0 = time.perf_counter()
    out = s.compute_tracks(*call, timing=True)
    runs.append((out[-1], time.perf_counter() - t0))
phase = np.median(np.array([r[0] for r in runs]), axis=0)
wall = float(np.median([r[1] for r in runs]))
start, length, kept, off, loc = out[:5]
print(f"problem: {F} frames {W}x{H}; {len(start)} tracks created, {int(kept.sum())} kept, {int(off[-1])} kept observations, "
      f"{int(length.sum()) / F:.0f} observations per frame")
names = ("candidates", "sort", "walk", "table")
print("kernel ms: " + ", ".join(f"{n} {m:.3f}" for n, m in zip(names, phase)) + f"; total {phase.sum():.3f}; "
      f"call {wall * 1e3:.1f} ms wall (walk {phase[2] / F * 1e3:.1f} us per frame)")
if not args.no_drop_in:
    lib_dir = os.path.dirname(_b.build_lib_python())
    sys.path.insert(0, lib_dir)
    lib = importlib.import_module("lib_python")
    tmp = tempfile.mkdtemp(prefix="tracks_bench_")
    try:
        base = dataset_io.write_dataset(os.path.join(tmp, "v"), v)
        dataset_io.write_flow_inputs(base, pairs, flow, mask, colors)
        dv = lib.DepthVideo()
        lib.DepthVideoImporter.importVideo(dv, base, True)
        p = lib.DepthVideoProcessor.Params()
        p.frameRange.fromString(f"0-{F - 1}")
        proc = lib.DepthVideoProcessor(dv)
        ops = []
        for _ in range(3):
            t0 = time.perf_counter()
            tt = proc.computeTracks(p)
            ops.append(time.perf_counter() - t0)
        assert tt.numTracks() == len(start)
        print(f"drop-in DepthVideoProcessor.computeTracks: {np.median(ops):.2f} s wall (median of 3, files included)")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
t0 = time.perf_counter()
ref = compute_tracks(corner, W, H, v.inv_aspect, active, 0, F - 1, flow, mask, present, None)
cpu = time.perf_counter() - t0
assert from_arrays(F, *out[:5]) == ref, "GPU tracks differ from the restatement"
print(f"numpy restatement: {cpu:.2f} s ({cpu / wall:.0f} x the GPU call); GPU result identical")
