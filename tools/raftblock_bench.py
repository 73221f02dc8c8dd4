"""Development aid (GPU): RAFT's whole update block (csrc/cvd_raftconv.h and csrc/cvd_raftgru.h,
robust_cvd_amd.raft_ops.BasicUpdateBlock) at the flow stage's working size: B = 1, 72 x 128 features (a 1024 x 576 input).

Kernel times are HIP-event times (median of --calls after warm-up, with min .. max): the twelve launches through the library's
timed entry point, the whole call through the module on torch's current stream.  FLOP = 2 M K N per layer; the share of the 157 TF
f32 matrix peak is what the times imply.  The baseline is what the parent commit offers: the same block written with stock torch
ops (cat, Conv2d, relu) with the project's SepConvGRU inside, on the same GPU, warmed up so that the vendor library's algorithm
search lies outside the timing; the two agree within the suite's bars (gross agreement checked here on the first call).  Each
layer of the baseline is also timed on its own (Conv2d + ReLU as torch runs them).  The loop figure is 20 x (lookup + block +
upsampling), one directed pair's refinement loop after the encoders, in alternating rounds in one process.  Seeded random inputs
(never zeros).
Usage: python tools/raftblock_bench.py [--out profiles/raftblock_bench.json] [--calls 20] [--h 72 --w 128]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from robust_cvd_amd import api
from robust_cvd_amd import torch_common as tc
from robust_cvd_amd.raft_ops import BasicUpdateBlock, CorrBlock, SepConvGRU, upsample_flow

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--h", type=int, default=72)
ap.add_argument("--w", type=int, default=128)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("raftblock_bench needs a GPU: there is nothing to measure without one")
dev = torch.device("cuda", 0)
B, H, W = 1, args.h, args.w
M = B * H * W
PEAK = 157e12


def layer_flop(name):
    o, c, kh, kw = api.raft_block_weight_shape(name)
    return 2.0 * M * c * kh * kw * o


# the twelve launches of cvd_raft_update_block_timed: (name, FLOP)
LAUNCHES = [("encoder.convc1", layer_flop("encoder.convc1")), ("encoder.convc2", layer_flop("encoder.convc2")),
            ("encoder.convf1", layer_flop("encoder.convf1")), ("encoder.convf2", layer_flop("encoder.convf2")),
            ("encoder.conv+flow_copy", layer_flop("encoder.conv")),
            ("gru.half1_zr", 2 * layer_flop("gru.convz1")), ("gru.half1_q_gate", layer_flop("gru.convq1")),
            ("gru.half2_zr", 2 * layer_flop("gru.convz2")), ("gru.half2_q_gate", layer_flop("gru.convq2")),
            ("flow_head.conv1|mask.0", layer_flop("flow_head.conv1") + layer_flop("mask.0")),
            ("flow_head.conv2", layer_flop("flow_head.conv2")), ("mask.2", layer_flop("mask.2"))]
FLOP_CALL = sum(f for _n, f in LAUNCHES)


class StockBlock(torch.nn.Module):
    """BasicUpdateBlock with stock torch ops as raft/core/update.py:96-114, 133-156 writes it, the project's SepConvGRU inside:
    the form the parent commit offers."""

    def __init__(self):
        super().__init__()
        enc = torch.nn.Module()
        enc.convc1 = torch.nn.Conv2d(324, 256, 1)
        enc.convc2 = torch.nn.Conv2d(256, 192, 3, padding=1)
        enc.convf1 = torch.nn.Conv2d(2, 128, 7, padding=3)
        enc.convf2 = torch.nn.Conv2d(128, 64, 3, padding=1)
        enc.conv = torch.nn.Conv2d(256, 126, 3, padding=1)
        self.encoder = enc
        self.gru = SepConvGRU(128, 256)
        head = torch.nn.Module()
        head.conv1 = torch.nn.Conv2d(128, 256, 3, padding=1)
        head.conv2 = torch.nn.Conv2d(256, 2, 3, padding=1)
        self.flow_head = head
        self.mask = torch.nn.Sequential(torch.nn.Conv2d(128, 256, 3, padding=1), torch.nn.ReLU(inplace=True),
                                        torch.nn.Conv2d(256, 576, 1))

    def forward(self, net, inp, corr, flow):
        e = self.encoder
        cor = F.relu(e.convc2(F.relu(e.convc1(corr))))
        flo = F.relu(e.convf2(F.relu(e.convf1(flow))))
        motion = torch.cat([F.relu(e.conv(torch.cat([cor, flo], dim=1))), flow], dim=1)
        net = self.gru(net, (inp, motion))
        delta_flow = self.flow_head.conv2(F.relu(self.flow_head.conv1(net)))
        return net, 0.25 * self.mask(net), delta_flow


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


torch.manual_seed(31700)
with torch.no_grad():
    stock = StockBlock().to(dev)
    block = BasicUpdateBlock().to(dev)
    block.load_state_dict(stock.state_dict())
    net = torch.tanh(torch.randn(B, 128, H, W, device=dev))
    inp = torch.relu(torch.randn(B, 128, H, W, device=dev))
    corr = 4 * torch.randn(B, 324, H, W, device=dev)
    flow = 2 * torch.randn(B, 2, H, W, device=dev)
    ins = (net, inp, corr, flow)

    for _ in range(5):          # the vendor library's algorithm search, outside every timing
        stock(*ins)
    torch.cuda.synchronize(dev)
    diffs = {n: float((a - b).abs().max()) for n, a, b in zip(("net", "mask", "delta_flow"), block(*ins), stock(*ins))}
    again = block(*ins)
    repeat_equal = all(bool(torch.equal(a, b)) for a, b in zip(again, block(*ins)))
    checks = {"max_abs_diff_to_stock_torch": diffs, "repeat_equal": repeat_equal}
    print("module against the torch baseline:", checks, flush=True)
    assert max(diffs.values()) < 1e-3 and repeat_equal, checks     # (gross agreement only: the bars are the suite's)

    result = {"shape": {"B": B, "H": H, "W": W, "pixels": M, "gflop_per_call": FLOP_CALL / 1e9},
              "checks": checks, "f32_matrix_peak_tflops": PEAK / 1e12}

    # the twelve launches, through the timed entry point (events around each launch on torch's stream, host waits)
    handle = tc.solver(dev)
    modules = [block.get_submodule(n) for n in api.UPDATE_BLOCK_PARAMETERS]
    w_table = (C.c_void_p * 15)(*[m.weight.data_ptr() for m in modules])
    b_table = (C.c_void_p * 15)(*[m.bias.data_ptr() for m in modules])
    net_out, delta_out = torch.empty_like(net), torch.empty_like(flow)
    mask_out = torch.empty(B, 576, H, W, device=dev)
    ms = (C.c_double * 12)()

    def timed():
        stream = torch.cuda.current_stream(dev).cuda_stream
        handle._check(handle._fn("raft_update_block_timed")(
            handle._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(324), C.c_int32(324), C.c_void_p(net.data_ptr()),
            C.c_void_p(inp.data_ptr()), C.c_void_p(corr.data_ptr()), C.c_void_p(flow.data_ptr()), w_table, b_table,
            C.c_void_p(net_out.data_ptr()), C.c_void_p(delta_out.data_ptr()), C.c_void_p(mask_out.data_ptr()), C.c_void_p(stream), ms))
        return list(ms)

    for _ in range(3):
        timed()
    per_launch = np.array([timed() for _ in range(args.calls)])
    result["launches"] = {n: with_rate(stats(per_launch[:, i], args.calls), f) for i, (n, f) in enumerate(LAUNCHES)}

    # the baseline's layers one by one, as torch runs them (Conv2d and its ReLU; the cat's are not in these figures)
    e, fh = stock.encoder, stock.flow_head
    cor1 = F.relu(e.convc1(corr))
    flo1 = F.relu(e.convf1(flow))
    cor_flo = torch.cat([F.relu(e.convc2(cor1)), F.relu(e.convf2(flo1))], dim=1)
    new_net = stock.gru(net, (inp, torch.cat([F.relu(e.conv(cor_flo)), flow], dim=1)))
    hidden_f, hidden_m = F.relu(fh.conv1(new_net)), F.relu(stock.mask[0](new_net))
    torch_layers = {
        "encoder.convc1": (lambda: F.relu(e.convc1(corr)), layer_flop("encoder.convc1")),
        "encoder.convc2": (lambda: F.relu(e.convc2(cor1)), layer_flop("encoder.convc2")),
        "encoder.convf1": (lambda: F.relu(e.convf1(flow)), layer_flop("encoder.convf1")),
        "encoder.convf2": (lambda: F.relu(e.convf2(flo1)), layer_flop("encoder.convf2")),
        "encoder.conv": (lambda: F.relu(e.conv(cor_flo)), layer_flop("encoder.conv")),
        "flow_head.conv1": (lambda: F.relu(fh.conv1(new_net)), layer_flop("flow_head.conv1")),
        "mask.0": (lambda: F.relu(stock.mask[0](new_net)), layer_flop("mask.0")),
        "flow_head.conv2": (lambda: fh.conv2(hidden_f), layer_flop("flow_head.conv2")),
        "mask.2": (lambda: 0.25 * stock.mask[2](hidden_m), layer_flop("mask.2")),
    }
    result["torch_layers"] = {n: with_rate(event_ms(fn, args.calls), f) for n, (fn, f) in torch_layers.items()}

    result["call"] = with_rate(event_ms(lambda: block(*ins), args.calls), FLOP_CALL)
    result["call_without_mask"] = event_ms(lambda: block(*ins, compute_mask=False), args.calls)
    result["call_torch"] = with_rate(event_ms(lambda: stock(*ins), args.calls), FLOP_CALL)

    # 20 x (lookup + block + upsampling): a directed pair's refinement loop after the encoders
    fmap1, fmap2 = torch.randn(B, 256, H, W, device=dev), torch.randn(B, 256, H, W, device=dev)
    corr_fn = CorrBlock(fmap1, fmap2, num_levels=4, radius=4)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev),
                            indexing="ij")
    coords0 = torch.stack([xs, ys], 0)[None].repeat(B, 1, 1, 1)

    def loop(update):
        n, coords1 = net, coords0.clone()
        for _ in range(args.iters):
            n, mask, delta = update(n, inp, corr_fn(coords1), coords1 - coords0)
            coords1 = coords1 + delta
            up = upsample_flow(coords1 - coords0, mask)
        return up

    loop_diff = float((loop(block) - loop(stock)).abs().max())
    rounds = {"module": [], "torch": []}
    for _ in range(args.rounds):                                   # alternating rounds in one process
        rounds["module"].append(event_ms(lambda: loop(block), 1, warmup=1)["ms_median"])
        rounds["torch"].append(event_ms(lambda: loop(stock), 1, warmup=1)["ms_median"])
    result["loop"] = {"iterations": args.iters, "rounds": args.rounds, "max_abs_diff_flow_up": loop_diff,
                      "module_ms": rounds["module"], "torch_ms": rounds["torch"],
                      "module_ms_median": float(np.median(rounds["module"])), "module_ms_min": float(np.min(rounds["module"])),
                      "module_ms_max": float(np.max(rounds["module"])),
                      "torch_ms_median": float(np.median(rounds["torch"])), "torch_ms_min": float(np.min(rounds["torch"])),
                      "torch_ms_max": float(np.max(rounds["torch"]))}
    result["loop"]["speedup"] = result["loop"]["torch_ms_median"] / result["loop"]["module_ms_median"]
    result["conditions"] = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
                            "timer": "HIP events", "not_profiled": "no counters, no per-kernel trace of the torch baseline"}

for n, _f in LAUNCHES:
    k = result["launches"][n]
    print(f"{n}: {k['ms_median']:.3f} ms (median of {k['calls']}, {k['ms_min']:.3f} .. {k['ms_max']:.3f}); {k['gflop']:.2f} GFLOP -> "
          f"{k['tflops']:.1f} TF = {100 * k['share_of_157tf']:.1f} % of 157 TF", flush=True)
for n, k in result["torch_layers"].items():
    print(f"torch {n}: {k['ms_median']:.3f} ms ({k['ms_min']:.3f} .. {k['ms_max']:.3f}); {k['tflops']:.1f} TF", flush=True)
c, t = result["call"], result["call_torch"]
print(f"call: module {c['ms_median']:.3f} ms ({c['ms_min']:.3f} .. {c['ms_max']:.3f}; {c['tflops']:.1f} TF, "
      f"{100 * c['share_of_157tf']:.1f} %), without the mask {result['call_without_mask']['ms_median']:.3f} ms; stock torch block with "
      f"the project's GRU {t['ms_median']:.3f} ms ({t['ms_min']:.3f} .. {t['ms_max']:.3f}; {t['tflops']:.1f} TF)", flush=True)
lp = result["loop"]
print(f"{lp['iterations']} x (lookup + block + upsampling): module {lp['module_ms_median']:.2f} ms ({lp['module_ms_min']:.2f} .. "
      f"{lp['module_ms_max']:.2f}), stock torch block {lp['torch_ms_median']:.2f} ms ({lp['torch_ms_min']:.2f} .. "
      f"{lp['torch_ms_max']:.2f}) (x {lp['speedup']:.2f}; medians of {lp['rounds']} alternating rounds; flow_up differs by "
      f"{lp['max_abs_diff_flow_up']:.2e})", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
print(json.dumps(result))
