"""Development aid (GPU): the SepConvGRU of RAFT's update block (csrc/cvd_raftgru.h, robust_cvd_amd.raft_ops.SepConvGRU) at the
flow stage's working size: B = 1, 72 x 128 features (a 1024 x 576 input), hidden 128, input 256.

Kernel times are HIP-event times (median of --calls after warm-up): the four launches through the library's timed entry point, the
whole call through the module on torch's current stream.  The arithmetic is 2 x 9216 x 1920 x 384 FLOP per half (27.2 GFLOP a
call at this size); the share of the 157 TF f32 matrix peak is what the times imply.  The baseline is the same module written with
stock torch ops (cat, Conv2d, sigmoid, tanh) on the same GPU, warmed up so that the vendor library's algorithm search lies outside
the timing; the two agree within the suite's bars (gross agreement checked here on the first call).  The loop figure is 20 x GRU
(one directed pair's refinement loop as far as this operator goes) in alternating rounds in one process.  Seeded random inputs
(never zeros).
Usage: python tools/raftgru_bench.py [--out profiles/raftgru_bench.json] [--calls 20] [--h 72 --w 128]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from robust_cvd_amd import api
from robust_cvd_amd import torch_common as tc
from robust_cvd_amd.raft_ops import SepConvGRU

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--h", type=int, default=72)
ap.add_argument("--w", type=int, default=128)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("raftgru_bench needs a GPU: there is nothing to measure without one")
dev = torch.device("cuda", 0)
B, H, W = 1, args.h, args.w
M = B * H * W
PEAK = 157e12
FLOP_HALF_ZR = 2.0 * M * 1920 * 256
FLOP_HALF_Q = 2.0 * M * 1920 * 128
FLOP_CALL = 2 * (FLOP_HALF_ZR + FLOP_HALF_Q)


class StockGRU(torch.nn.Module):
    """SepConvGRU(128, 256) with stock torch ops, as raft/core/update.py:37-75 writes it."""

    def __init__(self):
        super().__init__()
        for name in api.GRU_PARAMETERS:
            k = api.raft_gru_weight_shape(name)[2:]
            setattr(self, name, torch.nn.Conv2d(384, 128, k, padding=(k[0] // 2, k[1] // 2)))

    def forward(self, h, x):
        for half in ("1", "2"):
            hx = torch.cat([h, x], dim=1)
            z = torch.sigmoid(getattr(self, "convz" + half)(hx))
            r = torch.sigmoid(getattr(self, "convr" + half)(hx))
            q = torch.tanh(getattr(self, "convq" + half)(torch.cat([r * h, x], dim=1)))
            h = (1 - z) * h + z * q
        return h


def stats(times, calls):
    t = np.array(times)
    return {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max()), "calls": calls}


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
    return stats(times, calls)


def with_rate(stat, flop):
    stat = dict(stat, gflop=flop / 1e9)
    stat["tflops"] = flop / (stat["ms_median"] * 1e-3) / 1e12
    stat["share_of_157tf"] = flop / (stat["ms_median"] * 1e-3) / PEAK
    return stat


torch.manual_seed(20270)
with torch.no_grad():
    stock = StockGRU().to(dev)
    gru = SepConvGRU().to(dev)
    gru.load_state_dict(stock.state_dict())
    h = torch.tanh(torch.randn(B, 128, H, W, device=dev))
    inp = torch.relu(torch.randn(B, 128, H, W, device=dev))
    motion = torch.relu(torch.randn(B, 128, H, W, device=dev))
    x = torch.cat([inp, motion], dim=1)

    for _ in range(5):          # the vendor library's algorithm search, outside every timing
        stock(h, x)
    torch.cuda.synchronize(dev)
    diff = float((gru(h, x) - stock(h, x)).abs().max())
    segmented_equal = bool(torch.equal(gru(h, (inp, motion)), gru(h, x)))
    checks = {"max_abs_diff_to_stock_torch": diff, "segment_form_equal": segmented_equal}
    print("module against the torch baseline:", checks, flush=True)
    assert diff < 1e-4 and segmented_equal, checks     # (gross agreement only: the bars are the suite's)

    result = {"shape": {"B": B, "H": H, "W": W, "hidden": 128, "input": 256, "pixels": M, "gflop_per_call": FLOP_CALL / 1e9},
              "checks": checks, "f32_matrix_peak_tflops": PEAK / 1e12}

    # the four launches, through the timed entry point (events around each launch on torch's stream, then a host wait)
    handle = tc.solver(dev)
    out = torch.empty_like(h)
    weights = [getattr(gru, n).weight for n in api.GRU_PARAMETERS]
    biases = [getattr(gru, n).bias for n in api.GRU_PARAMETERS]
    seg_table, seg_channels = (C.c_void_p * 1)(x.data_ptr()), (C.c_int32 * 1)(256)
    w_table = (C.c_void_p * 6)(*[t.data_ptr() for t in weights])
    b_table = (C.c_void_p * 6)(*[t.data_ptr() for t in biases])
    ms = (C.c_double * 4)()

    def timed():
        stream = torch.cuda.current_stream(dev).cuda_stream
        handle._check(handle._fn("raft_sepconv_gru_timed")(handle._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_void_p(h.data_ptr()),
                                                           C.c_int32(1), seg_table, seg_channels, w_table, b_table,
                                                           C.c_void_p(out.data_ptr()), C.c_void_p(stream), ms))
        return list(ms)

    for _ in range(3):
        timed()
    per_launch = np.array([timed() for _ in range(args.calls)])
    names = ("half1_zr", "half1_q_gate", "half2_zr", "half2_q_gate")
    flops = (FLOP_HALF_ZR, FLOP_HALF_Q, FLOP_HALF_ZR, FLOP_HALF_Q)
    result["launches"] = {n: with_rate(stats(per_launch[:, i], args.calls), f) for i, (n, f) in enumerate(zip(names, flops))}
    result["call"] = with_rate(event_ms(lambda: gru(h, x), args.calls), FLOP_CALL)
    result["call_segmented"] = with_rate(event_ms(lambda: gru(h, (inp, motion)), args.calls), FLOP_CALL)
    result["call_torch"] = with_rate(event_ms(lambda: stock(h, x), args.calls), FLOP_CALL)
    result["call_torch_with_cat"] = event_ms(lambda: stock(h, torch.cat([inp, motion], dim=1)), args.calls)

    def loop_module():
        s = h
        for _ in range(args.iters):
            s = gru(s, (inp, motion))

    def loop_torch():
        s = h
        for _ in range(args.iters):
            s = stock(s, torch.cat([inp, motion], dim=1))

    rounds = {"module": [], "torch": []}
    for _ in range(args.rounds):                                   # alternating rounds in one process
        rounds["module"].append(event_ms(loop_module, 1, warmup=1)["ms_median"])
        rounds["torch"].append(event_ms(loop_torch, 1, warmup=1)["ms_median"])
    result["loop"] = {"iterations": args.iters, "rounds": args.rounds,
                      "module_ms": rounds["module"], "torch_ms": rounds["torch"],
                      "module_ms_median": float(np.median(rounds["module"])), "module_ms_min": float(np.min(rounds["module"])),
                      "module_ms_max": float(np.max(rounds["module"])),
                      "torch_ms_median": float(np.median(rounds["torch"])), "torch_ms_min": float(np.min(rounds["torch"])),
                      "torch_ms_max": float(np.max(rounds["torch"]))}
    result["loop"]["speedup"] = result["loop"]["torch_ms_median"] / result["loop"]["module_ms_median"]
    result["conditions"] = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
                            "timer": "HIP events", "not_profiled": "no counters, no per-kernel trace of the torch baseline"}

for n in names:
    k = result["launches"][n]
    print(f"{n}: {k['ms_median']:.3f} ms (median of {k['calls']}, {k['ms_min']:.3f} .. {k['ms_max']:.3f}); {k['gflop']:.2f} GFLOP -> "
          f"{k['tflops']:.1f} TF = {100 * k['share_of_157tf']:.1f} % of 157 TF", flush=True)
c, t = result["call"], result["call_torch"]
print(f"call: module {c['ms_median']:.3f} ms ({c['tflops']:.1f} TF, {100 * c['share_of_157tf']:.1f} %), segmented "
      f"{result['call_segmented']['ms_median']:.3f} ms; torch ops {t['ms_median']:.3f} ms ({t['tflops']:.1f} TF), with the cat of x "
      f"{result['call_torch_with_cat']['ms_median']:.3f} ms", flush=True)
lp = result["loop"]
print(f"{lp['iterations']} x GRU: module {lp['module_ms_median']:.2f} ms ({lp['module_ms_min']:.2f} .. {lp['module_ms_max']:.2f}), torch ops "
      f"{lp['torch_ms_median']:.2f} ms ({lp['torch_ms_min']:.2f} .. {lp['torch_ms_max']:.2f}) (x {lp['speedup']:.2f}; medians of "
      f"{lp['rounds']} alternating rounds)", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
print(json.dumps(result))
