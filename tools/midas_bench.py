"""Development aid (GPU): the decoder of MiDaS v2.1 (csrc/cvd_midas.h, robust_cvd_amd.midas.MidasNet) at the depth stage's working
size: 384 x 224 frames (feature maps 96 x 56 down to 12 x 7), B = 1 and B = 8, features = 256.

Times are HIP-event times (median of --calls after warm-up, with min .. max): every launch of the decoder through the library's
timed entry point with its GFLOP (2 M K N per convolution; the share of the 157 TF f32 matrix peak is what the times imply); the
whole call through MidasNet.decode on torch's current stream against a stock-torch decoder with the same weights, written with the
in-place semantics of the reference's ResidualConvUnit (its skip adds relu(x)), in alternating rounds in one process, warmed up so
that the vendor library's algorithm search lies outside the timing; and the convolutions that split K (layer4_rn, layer3_rn, one of
refinenet4) at S = 1 against the rule's S through cvd_midas_conv_device.  Seeded random inputs (never zeros).  The backbone is not
part of any figure: the feature maps are inputs.
Usage: python tools/midas_bench.py [--out profiles/midas_bench.json] [--calls 20] [--rounds 5]"""
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
from robust_cvd_amd import midas
from robust_cvd_amd import torch_common as tc

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--height", type=int, default=224)
ap.add_argument("--width", type=int, default=384)
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("midas_bench needs a GPU: there is nothing to measure without one")
if args.height % 32 or args.width % 32:
    sys.exit("height and width must be multiples of 32")
dev = torch.device("cuda", 0)
H, W = args.height, args.width
PEAK = 157e12
FEATURES = 256
CHANNELS = api.MIDAS_BACKBONE_CHANNELS
SIZES = [(H >> (k + 2), W >> (k + 2)) for k in range(4)]


def conv_level(name):
    """(level 0 .. 3 of the feature maps, or 4 = twice level 0) a convolution of the weight table runs at."""
    if name.endswith("_rn"):
        return int(name[5]) - 1
    return 4 if name == "output_conv.0" else int(name[9]) - 1


def conv_flops(batch):
    """FLOP of the 19 convolutions of the weight table and of the head, for `batch` images."""
    out = []
    for name in api.MIDAS_PARAMETERS[:19]:
        o, c, k, _ = api.midas_weight_shape(name, FEATURES)
        level = conv_level(name)
        h, w = (2 * SIZES[0][0], 2 * SIZES[0][1]) if level == 4 else SIZES[level]
        out.append(2.0 * batch * h * w * c * k * k * o)
    head = 2.0 * batch * H * W * (128 * 9 * 32 + 32)
    return out, head


def stock_unit(x, conv1, conv2):
    r = F.relu(x)
    return conv2(F.relu(conv1(r))) + r          # the reference's in-place ReLU: the skip is relu(x)


def stock_decoder(net, maps):
    s = net.scratch
    rn = [F.conv2d(m, getattr(s, f"layer{k + 1}_rn").weight, None, padding=1) for k, m in enumerate(maps)]
    path = None
    for k in (4, 3, 2, 1):
        block = getattr(s, f"refinenet{k}")
        out = rn[k - 1]
        if path is not None:
            out = path + stock_unit(out, *conv_pair(block.resConfUnit1))
        out = stock_unit(out, *conv_pair(block.resConfUnit2))
        path = F.interpolate(out, scale_factor=2, mode="bilinear", align_corners=True)
    oc = s.output_conv
    y = F.interpolate(F.conv2d(path, oc[0].weight, oc[0].bias, padding=1), scale_factor=2, mode="bilinear", align_corners=False)
    y = F.conv2d(F.relu(F.conv2d(y, oc[2].weight, oc[2].bias, padding=1)), oc[4].weight, oc[4].bias)
    return F.relu(y).squeeze(1)


def conv_pair(unit):
    return (lambda t: F.conv2d(t, unit.conv1.weight, unit.conv1.bias, padding=1),
            lambda t: F.conv2d(t, unit.conv2.weight, unit.conv2.bias, padding=1))


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
    if flop > 0 and stat["ms_median"] > 0:
        stat["tflops"] = flop / (stat["ms_median"] * 1e-3) / 1e12
        stat["share_of_157tf"] = flop / (stat["ms_median"] * 1e-3) / PEAK
    return stat


torch.manual_seed(31900)
result = {"shape": {"height": H, "width": W, "features": FEATURES, "feature_maps": SIZES}, "f32_matrix_peak_tflops": PEAK / 1e12, "batches": {}}
with torch.no_grad():
    backbone = torch.nn.Module()          # never run: the feature maps are the inputs here
    for k in (1, 2, 3, 4):
        setattr(backbone, f"layer{k}", torch.nn.Identity())
    net = midas.MidasNet(features=FEATURES, backbone=backbone).to(dev).eval()
    handle = tc.solver(dev)
    convs = [net.scratch.get_submodule(n) for n in api.MIDAS_PARAMETERS]
    w_table = (C.c_void_p * 21)(*[m.weight.data_ptr() for m in convs])
    b_table = (C.c_void_p * 17)(*[m.bias.data_ptr() for m in convs[4:]])

    for batch in args.batches:
        # features as a ReLU network gives them, with a negative part behind the layerK_rn convolutions
        maps = [torch.relu(torch.randn(batch, c, h, w, device=dev)).contiguous() for c, (h, w) in zip(CHANNELS, SIZES)]
        for _ in range(5):          # the vendor library's algorithm search, outside every timing
            stock_decoder(net, maps)
        torch.cuda.synchronize(dev)
        ours, stock = net.decode(*maps), stock_decoder(net, maps)
        checks = {"max_abs_diff_to_stock_torch": float((ours - stock).abs().max()), "output_scale": float(stock.abs().max()),
                  "repeat_equal": bool(torch.equal(net.decode(*maps), ours))}
        print(f"B = {batch}: decoder against the torch baseline:", checks, flush=True)
        assert checks["max_abs_diff_to_stock_torch"] < 1e-3 * max(checks["output_scale"], 1.0) and checks["repeat_equal"]
        entry = {"checks": checks}

        out = torch.empty(batch, H, W, device=dev)
        ms = (C.c_double * api.MIDAS_TIMED_SLOTS)()
        m_table = (C.c_void_p * 4)(*[t.data_ptr() for t in maps])

        def timed():
            stream = torch.cuda.current_stream(dev).cuda_stream
            handle._check(handle._fn("midas_decoder_timed")(
                handle._h, C.c_int32(batch), C.c_int32(FEATURES), (C.c_int32 * 4)(*CHANNELS), (C.c_int32 * 4)(*[s[0] for s in SIZES]),
                (C.c_int32 * 4)(*[s[1] for s in SIZES]), m_table, w_table, b_table, C.c_int32(1), C.c_void_p(out.data_ptr()),
                C.c_void_p(stream), ms))
            return list(ms)
        for _ in range(3):
            timed()
        per_launch = np.array([timed() for _ in range(args.calls)])
        flops, head_flop = conv_flops(batch)
        launches = {}
        for i, name in enumerate(api.MIDAS_PARAMETERS[:19]):
            level = conv_level(name)
            h, w = (2 * SIZES[0][0], 2 * SIZES[0][1]) if level == 4 else SIZES[level]
            launches[name] = dict(with_rate(stats(per_launch[:, 2 * i], args.calls), flops[i]),
                                  split=api.midas_split(api.midas_weight_shape(name, FEATURES)[1] * 9, h * w))
            if per_launch[:, 2 * i + 1].max() > 0:
                launches[name + ":fold"] = stats(per_launch[:, 2 * i + 1], args.calls)
        for j, name in enumerate(("refinenet4:upsample", "refinenet3:upsample", "refinenet2:upsample", "refinenet1:upsample", "output_conv.1:upsample")):
            launches[name] = stats(per_launch[:, 38 + j], args.calls)
        launches["head"] = with_rate(stats(per_launch[:, 43], args.calls), head_flop)
        entry["launches"] = launches
        entry["sum_of_launches"] = with_rate(stats(per_launch.sum(axis=1), args.calls), sum(flops) + head_flop)
        entry["convolutions_ms_median"] = float(np.median(per_launch[:, 0:38:2].sum(axis=1)))
        entry["folds_ms_median"] = float(np.median(per_launch[:, 1:38:2].sum(axis=1)))
        entry["upsamplings_ms_median"] = float(np.median(per_launch[:, 38:43].sum(axis=1)))

        # the whole call against stock torch: alternating rounds in one process
        rounds = {"module": [], "torch": []}
        for _ in range(args.rounds):
            rounds["module"].append(event_ms(lambda: net.decode(*maps), args.calls, warmup=2)["ms_median"])
            rounds["torch"].append(event_ms(lambda: stock_decoder(net, maps), args.calls, warmup=2)["ms_median"])
        entry["call"] = {"rounds": args.rounds, "calls_per_round": args.calls, "module_ms": rounds["module"], "torch_ms": rounds["torch"],
                         "gflop": (sum(flops) + head_flop) / 1e9}
        for k in ("module", "torch"):
            t = np.array(rounds[k])
            entry["call"].update({f"{k}_ms_median": float(np.median(t)), f"{k}_ms_min": float(t.min()), f"{k}_ms_max": float(t.max())})
        entry["call"]["torch_over_module"] = entry["call"]["torch_ms_median"] / entry["call"]["module_ms_median"]

        # S = 1 against the rule's S, conv + fold, through the single-convolution entry point
        split = {}
        for name, level in (("layer4_rn", 3), ("layer3_rn", 2), ("refinenet4.resConfUnit2.conv1", 3)):
            conv = net.scratch.get_submodule(name)
            o, c, _k, _ = conv.weight.shape
            h, w = SIZES[level]
            x = maps[level] if name.endswith("_rn") else torch.randn(batch, c, h, w, device=dev)
            y = torch.empty(batch, o, h, w, device=dev)
            S = api.midas_split(c * 9, h * w)

            def run(forced):
                stream = torch.cuda.current_stream(dev).cuda_stream
                handle._check(handle._fn("midas_conv_device")(
                    handle._h, C.c_int32(batch), C.c_int32(h), C.c_int32(w), C.c_int32(c), C.c_int32(o), C.c_int32(3), C.c_void_p(x.data_ptr()),
                    C.c_void_p(conv.weight.data_ptr()), None if conv.bias is None else C.c_void_p(conv.bias.data_ptr()), C.c_int32(0),
                    C.c_int32(0), None, C.c_int32(0), None, C.c_int32(forced), C.c_void_p(y.data_ptr()), C.c_void_p(stream)))
            flop = 2.0 * batch * h * w * c * 9 * o
            split[name] = {"S": S, "unsplit": with_rate(event_ms(lambda: run(1), args.calls), flop),
                           "split": with_rate(event_ms(lambda: run(S), args.calls), flop)}
            split[name]["unsplit_over_split"] = split[name]["unsplit"]["ms_median"] / split[name]["split"]["ms_median"]
        entry["split_k"] = split
        result["batches"][str(batch)] = entry

    result["conditions"] = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
                            "timer": "HIP events",
                            "not_verified": "the trained checkpoint midas_v21-f6b98070.pt and the torchvision ResNeXt backbone (torchvision "
                                            "is not installed where this ran): weights are torch's default initialisation, the feature "
                                            "maps relu(N(0, 1))",
                            "not_profiled": "no counters, no per-kernel trace of the torch baseline"}

for batch, entry in result["batches"].items():
    for n, k in entry["launches"].items():
        rate = f"; {k['gflop']:.2f} GFLOP -> {k['tflops']:.1f} TF = {100 * k['share_of_157tf']:.1f} % of 157 TF" if "tflops" in k else ""
        print(f"B = {batch} {n}: {k['ms_median']:.3f} ms (median of {k['calls']}, {k['ms_min']:.3f} .. {k['ms_max']:.3f}){rate}", flush=True)
    c = entry["call"]
    print(f"B = {batch}: launches {entry['sum_of_launches']['ms_median']:.3f} ms (convolutions {entry['convolutions_ms_median']:.3f}, folds "
          f"{entry['folds_ms_median']:.3f}, upsamplings {entry['upsamplings_ms_median']:.3f}); call {c['module_ms_median']:.3f} ms "
          f"({c['module_ms_min']:.3f} .. {c['module_ms_max']:.3f}); stock torch {c['torch_ms_median']:.3f} ms ({c['torch_ms_min']:.3f} .. "
          f"{c['torch_ms_max']:.3f}); torch / module = {c['torch_over_module']:.2f} (medians of {c['rounds']} alternating rounds)", flush=True)
    for n, k in entry["split_k"].items():
        print(f"B = {batch} {n}: S = 1 {k['unsplit']['ms_median']:.3f} ms, S = {k['S']} {k['split']['ms_median']:.3f} ms "
              f"(x {k['unsplit_over_split']:.2f})", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
print(json.dumps(result))
