"""Development aid (GPU): the epipolar RANSAC (cvd_epipolar.h, setStaticFlagFromRansac) on the benchmark problem: 300 frames of
384 x 224, the 4140-pair flow list (synth.make_video(..., extra_offsets=6)), K = 1024.  Kernel times per phase from HIP events
(host<->device copies excluded), median of 5 calls.  A distance evaluation = one (hypothesis, constraint) test of both
point-to-line distances; 33 f64 flops each as written (14 fma + 5 mul), so f64 fraction = 33 x evaluations / score time over
the 78.6 TF f64 vector peak.  The CPU figure is the numpy restatement (tests/epipolar_reference.py) on a few pairs,
extrapolated linearly to every pair.  Usage: python tools/epipolar_bench.py"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from robust_cvd_amd import api, synth
from tests import epipolar_reference as er

F, W, H, K = 300, 384, 224, 1024
v = synth.make_video(F, W, H, seed=1234, extra_offsets=6)
P, C = len(v.pairs), v.num_constraints
print(f"problem: {F} frames {W}x{H}, {P} pairs, {C / 1e6:.2f} M constraints, K = {K}")
s = api.Solver(0)
s.epipolar_static_flags(v.offsets[:9], v.loc[:int(v.offsets[8])], W, 2.0, K)   # warm-up
runs = []
for _ in range(5):
    t0 = time.perf_counter()
    flags, Fm, best, ms = s.epipolar_static_flags(v.offsets, v.loc, W, 2.0, K, timing=True)
    runs.append((ms, time.perf_counter() - t0))
phase = np.median(np.array([r[0] for r in runs]), axis=0)
wall = float(np.median([r[1] for r in runs]))
names = ("normalise", "hypotheses", "score", "select")
evals = float(C) * K
print("kernel ms: " + ", ".join(f"{n} {m:.3f}" for n, m in zip(names, phase)) + f"; total {phase.sum():.3f}; call {wall * 1e3:.1f} ms wall")
print(f"score: {evals / 1e9:.2f} G distance evaluations, {evals / (phase[2] * 1e-3) / 1e9:.0f} G/s, "
      f"{33 * evals / (phase[2] * 1e-3) / 78.6e12 * 100:.1f} % of the f64 vector peak")
print(f"static fraction {flags.mean():.4f}; pairs with a valid F {int((best[:, 0] >= 0).sum())} / {P}")
sub = 4
t0 = time.perf_counter()
er.epipolar_static_flags(v.offsets, v.loc, W, 2.0, K, pairs=range(sub))
cpu = (time.perf_counter() - t0) / sub * P
print(f"numpy restatement: {cpu:.0f} s extrapolated from {sub} pairs ({cpu / wall:.0f} x the GPU call)")
