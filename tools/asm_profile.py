"""Development aid (GPU): phase timestamps of k_assemble_fast per part, and how a wave's constraint loop divides between its three
waits per unit and the walk (cvd_assembly.h: ASM_STAMP, ASM_WAIT_*).  Library variant with the stamps (100 MHz wall clock):
    python -c "from robust_cvd_amd import build; build.build_variant('asmprof', ['CVD_ASM_PROFILE'], ['cvd_eval'])"
then  python tools/asm_profile.py [headline | bilinear | bicubic [variant]]
headline: the workload of bench.py (300 frames, 4140 pairs, 17 x 10 grid) at the state its timed solves start from."""
import os, sys, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.cuda.init()
from robust_cvd_amd import api, synth
api.load_library(variant=sys.argv[2] if len(sys.argv) > 2 else "asmprof")  # (before bench / Solver load the product library)
from robust_cvd_amd.ctypes_types import *
mode = sys.argv[1] if len(sys.argv) > 1 else "headline"
p = OptParams.defaults()
if mode == "headline":
    import bench
    v = synth.make_video(300, 384, 224, seed=bench.SEED, extra_offsets=6)
    s = api.Solver(0)
    bench.prepare(s, v, p)
else:
    F = 300 if mode == "bilinear" else 100
    v = synth.make_video(F, 384, 224, seed=1234)
    s = api.Solver(0); synth.load_into(s, v)
    s.reset_spatial_xforms(XformDesc.spatial())
    s.reset_depth_xforms(XformDesc.grid_depth(17, 10) if mode == "bilinear" else XformDesc.grid_depth(4, 4, cubic=True))
for _ in range(3):
    s.evaluate(p, 0.1, None)
print("assembly launch", {k: v for k, v in s.assembly_launch_debug().items() if k != "cost_frame"})
lib = api.load_library()
buf = (C.c_ulonglong * (2048 * 16))()
assert lib.cvd_debug_asm_profile(buf) == 0
a = np.frombuffer(buf, dtype=np.uint64).reshape(2048, 16).astype(np.int64)
live = a[:, 0] > 0
wbuf = (C.c_ulonglong * (2048 * 64))()
assert lib.cvd_debug_asm_waits(wbuf) == 0
w = np.frombuffer(wbuf, dtype=np.uint64).reshape(2048, 8, 8).astype(np.int64)[live]
a = a[live]
t0 = a[:, 0].min()
us = lambda x: x / 100.0  # 100 MHz
end = a.max(1)
print("parts", len(a), "kernel span us", us(end.max() - t0))
st = us(a[:, 0] - t0)
print("start offsets us: median/max", np.median(st), st.max(), " started late (>30us):", int(np.sum(st > 30)))
first = st <= 30
print(f"first round: {int(first.sum())} parts end at median {np.median(us(end[first] - t0)):.1f} max {us(end[first] - t0).max():.1f};"
      f" later rounds: {int((~first).sum())} parts" + (f", life median {np.median(us(end[~first] - a[~first, 0])):.1f}" if (~first).any() else ""))
for name, (i, j) in {"zero": (0, 1), "loop(all waves)": (1, 2)}.items():
    x = us(a[:, j] - a[:, i]); print(f"{name:18s} min {x.min():8.1f} median {np.median(x):8.1f} max {x.max():8.1f}")
x = us(end - a[:, 2]); print(f"{'after loop':18s} min {x.min():8.1f} median {np.median(x):8.1f} max {x.max():8.1f}")
x = us(end - a[:, 0]); print(f"{'total':18s} min {x.min():8.1f} median {np.median(x):8.1f} max {x.max():8.1f}  sum/256 {x.sum()/256:8.1f}")
one = a[(a[:, 3] > 0) & (a[:, 3] >= a[:, 15])]   # (parts that reached the write-out in this launch)
for name, (i, j) in {"reduce PP": (2, 13), "shared": (13, 14), "regulariser": (14, 15), "cost+combine (fold)": (15, 3), "writeout": (3, 12)}.items():
    x = us(one[:, j] - one[:, i]); print(f"{name:18s} min {x.min():8.1f} median {np.median(x):8.1f} max {x.max():8.1f}")
# the waves' own loops: stamp 4 + wave is the wave's end of the loop, w[part, wave] = {wait 1, wait 2, wait 3, walk, count} summed over the
# wave's units (unit walk) or segments (segment walk: waits 1 and 2 do not exist, wait 3 is what a segment waits for at its top)
units = w[:, :, 4]
if units.sum() > 0:
    busy = units > 0
    names = ("wait: unit descriptor", "wait: pair frames / offsets", "wait: constants + staging + record", "walk")
    tot = w[:, :, :4].sum(axis=(0, 1)).astype(np.float64)
    print(f"waves with units / segments {int(busy.sum())} of {busy.size}; per wave median {np.median(units[busy]):.0f} max {units.max()}; in all {int(units.sum())}")
    for k, nme in enumerate(names):
        per = w[:, :, k][busy] / units[busy]
        print(f"{nme:36s} per unit / segment us: median {np.median(us(per)):6.2f} mean {us(tot[k]) / units.sum():6.2f}   share of the waves' loop time {tot[k] / tot.sum():6.1%}")
    waits = w[:, :, :3].sum(axis=2)
    loop = us(a[:, 4:12] - a[:, 1:2])  # each wave's loop phase, from the barrier behind the zeroing
    print(f"three waits together: {tot[:3].sum() / tot.sum():.1%} of the waves' loop time; per part (sum over waves) median {np.median(waits.sum(1) / np.maximum(1, w[:, :, :4].sum(axis=(1, 2)))):.1%}")
    print(f"a wave's loop phase us: median {np.median(loop[busy]):.1f} max {loop[busy].max():.1f}; stamped time in it median {np.median(us(w[:, :, :4].sum(2))[busy]):.1f}")
