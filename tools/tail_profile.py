#!/usr/bin/env python3
"""Development aid (GPU): where the workgroups of k_pcg_tail (finish + update of a PCG iteration in one launch) spend their life.
Library variant with wall-clock stamps (100 MHz):
    python -c "from robust_cvd_amd import build; build.build_variant('tailprof', ['CVD_TAIL_PROFILE'], ['cvd_matvec'])"
then  python tools/tail_profile.py [pairs_level [variant [nostage | closing]]]
(variant: another stamped library lib/libcvd_hip_<variant>.so, e.g. of a tree with one step taken out; nostage: the levels' rows
from memory behind the barrier, cvd_debug_options::tail_no_row_staging; closing: the tail sums its r^T z shares and finishes the
scalars itself, cvd_debug_options::tail_closes_scalars -- the default leaves them to the next product and the launch ends with its
slowest workgroup's share)"""
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.cuda.init()
from robust_cvd_amd import api, synth
api.load_library(variant=sys.argv[2] if len(sys.argv) > 2 else "tailprof")  # (before bench / Solver load the product library)
import bench
from robust_cvd_amd.ctypes_types import OptParams

level = int(sys.argv[1]) if len(sys.argv) > 1 else 6
v = synth.make_video(300, 384, 224, seed=bench.SEED, extra_offsets=level)
s = api.Solver(0)
p = OptParams.defaults()
bench.prepare(s, v, p)
# every launch that leaves stamps must be a working one.  Lockstep would do (no launch is enqueued past convergence) but keeps
# the closing tail; an iteration cap below the count a solve of this level needs does the same for both modes.
s.set_options(pcg_max_iterations=12)
if len(sys.argv) > 3 and sys.argv[3] == "nostage":
    s.set_options(tail_no_row_staging=1)
if len(sys.argv) > 3 and sys.argv[3] == "closing":
    s.set_options(tail_closes_scalars=1)
p.max_iterations = 2
s.pose_optimization_step(p, p.depth_deform_reg_final, convert_poses=False)   # the stamps of the LAST tail launch stay
lib = api.load_library()
buf = (C.c_ulonglong * (1024 * 16))()
assert lib.cvd_debug_tail_profile(buf) == 0
a = np.frombuffer(buf, dtype=np.uint64).reshape(1024, 16).astype(np.int64)   # (16 stamp slots per workgroup: cvd_pcg.h TAIL_STAMP)
a = a[a[:, 0] > 0]
F = v.num_frames
t0 = a[:, 0].min()
us = lambda x: x / 100.0
print("workgroups", len(a), " launch span us %.1f" % us(a[:, 4].max() - t0), " path", s.path_info())
if a[:, 10].min() > 0:   # (slot 10: the first wave has its ticket; the workgroup that drew the last one has written the release records)
    last = a[:, 1].argmax()
    print("slowest finish half ends at %.2f (workgroup %d), its arrival is done at %.2f, release seen at: median %.2f max %.2f"
          % (us(a[last, 1] - t0), last, us(a[last, 10] - t0), us(np.median(a[:, 3]) - t0), us(a[:, 3].max() - t0)))
# workgroups behind the frames': the exact dense level's (two frames each; none with the temporal pose level), then the temporal
# levels' (45 hats of the depth-grid level, 8 modes of the temporal pose level)
nExtra = len(a) - F
nD = (F + 1) // 2 if nExtra >= (F + 1) // 2 else 0
groups = [("frame workgroups", a[:F]), ("dense-level workgroups", a[F:F + nD])]
rest = a[F + nD:]
dbg = s.temporal_debug()
nTl = dbg["S"] * max(1, (dbg["nn"] - 1 + 9) // 10) if dbg else 0   # (hats x node ranges of 10 intervals: TlStep::parts)
groups += [("depth-grid level's workgroups", rest[:nTl]), ("temporal pose level's workgroups", rest[nTl:])]
for name, rows in groups:
    if not len(rows):
        continue
    print(name, len(rows))
    for label, x in (("start offset", us(rows[:, 0] - t0)), ("finish half", us(rows[:, 1] - rows[:, 0])),
                     ("operand requests", us(rows[:, 2] - rows[:, 1])), ("grid barrier + alpha", us(rows[:, 3] - rows[:, 2])),
                     ("update half", us(rows[:, 4] - rows[:, 3])), ("barrier release at", us(rows[:, 3] - t0)),
                     ("end at", us(rows[:, 4] - t0))):
        print(f"  {label:22s} min {x.min():6.2f}  median {np.median(x):6.2f}  mean {x.mean():6.2f}  max {x.max():6.2f}")
    if rows[:, 10].min() > 0:
        x = us(rows[:, 10] - rows[:, 1])
        print(f"  {'  drain + ticket':22s} min {x.min():6.2f}  median {np.median(x):6.2f}  mean {x.mean():6.2f}  max {x.max():6.2f}")
    if "level's" in name and rows[:, 8].min() > 0:
        x = us(rows[:, 8] - rows[:, 10])
        print(f"  {'  rows staged after':22s} min {x.min():6.2f}  median {np.median(x):6.2f}  mean {x.mean():6.2f}  max {x.max():6.2f}")
        x = us(rows[:, 4] - rows[:, 3])
        print(f"  {'  post-barrier chain':22s} min {x.min():6.2f}  median {np.median(x):6.2f}  mean {x.mean():6.2f}  max {x.max():6.2f}")
    if "level's" in name and rows[:, 5].min() > 0:   # (tlLevelRows' own stamps)
        for label, x in (("  node sums (q_T)", us(rows[:, 5] - rows[:, 3])), ("  rows + update", us(rows[:, 6] - rows[:, 5])),
                         ("  interpolation + share", us(rows[:, 7] - rows[:, 6])),
                         ("  ticket (closing tail)", us(rows[:, 4] - rows[:, 7]))):
            print(f"  {label:22s} min {x.min():6.2f}  median {np.median(x):6.2f}  mean {x.mean():6.2f}  max {x.max():6.2f}")
