"""Development aid (GPU): the ResNeXt-101 32x8d backbone of MiDaS v2.1 (csrc/cvd_resnext.h, robust_cvd_amd.midas.ResNeXt) and the whole
MidasNet at the depth stage's working size: 384 x 224 frames, B = 1 and B = 8.

Times are HIP-event times.  Every launch of the backbone through the library's timed entry point (median of --calls after warm-up,
with min .. max) with its GFLOP from the layer shapes (2 M K N per convolution; the share of the 157 TF f32 peak is what the times
imply).  The backbone call through midas.ResNeXt against the SAME backbone in stock torch ops -- the module's own nn.Conv2d(groups=32),
nn.BatchNorm2d in eval mode and nn.MaxPool2d called as torch modules under no_grad, so the weights are the same tensors --, and the
whole MidasNet.forward with the native backbone against the parent commit's form (that stock backbone inside MidasNet, the decoder on
the library in both).  The comparisons run in alternating rounds in one process, warmed up so that the vendor library's algorithm
search lies outside the timing, and report the median and min .. max of the rounds' medians plus the largest difference of the two
forms' outputs.  The baseline is always the stock-torch form measured in the same run.  Seeded random weights (He-scaled; a block's
last norm U(0.2, 0.5)) and inputs, never zeros.
Usage: python tools/midasnet_bench.py [--out profiles/midasnet_bench.json] [--calls 20] [--rounds 5]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

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
    sys.exit("midasnet_bench needs a GPU: there is nothing to measure without one")
if args.height % 32 or args.width % 32:
    sys.exit("height and width must be multiples of 32")
dev = torch.device("cuda", 0)
H, W = args.height, args.width
PEAK = 157e12
BLOCKS, GROUPS, WIDTH_PER_GROUP = api.RESNEXT101_32X8D
TABLE = api.resnext_conv_table(BLOCKS, GROUPS, WIDTH_PER_GROUP)


def conv_sizes():
    """Per convolution of TABLE: (input height, input width, output height, output width)."""
    out = [(H, W, H // 2, W // 2)]
    h, w = H // 4, W // 4
    block_in = (h, w)
    for c in TABLE[1:]:
        if c.name.endswith("conv1"):
            block_in = (h, w)
        hin, win = block_in if c.name.endswith("downsample.0") else (h, w)
        ho, wo = (hin - 1) // c.stride + 1, (win - 1) // c.stride + 1
        out.append((hin, win, ho, wo))
        h, w = ho, wo
    return out


SIZES = conv_sizes()


def conv_flop(i, batch):
    c, (_h, _w, ho, wo) = TABLE[i], SIZES[i]
    return 2.0 * batch * ho * wo * (c.in_channels // c.groups) * c.kernel_size ** 2 * c.out_channels


def stock_block(block, x):
    identity = x
    out = torch.relu_(block.bn1(block.conv1(x)))
    out = torch.relu_(block.bn2(block.conv2(out)))
    out = block.bn3(block.conv3(out))
    if block.downsample is not None:
        identity = block.downsample[1](block.downsample[0](x))
    out += identity
    return torch.relu_(out)


class StockStage(torch.nn.Module):
    """A stage of the native backbone's parameter holders run as the stock torch modules they are."""

    def __init__(self, stage, stem=None):
        super().__init__()
        self.stage, self.stem = stage, stem

    def forward(self, x):
        if self.stem is not None:
            conv, bn, _relu, pool = self.stem
            x = pool(torch.relu_(bn(conv(x))))
        for block in self.stage:
            x = stock_block(block, x)
        return x


def stock_backbone_of(rx):
    backbone = torch.nn.Module()
    backbone.layer1 = StockStage(rx.layer1[4], [rx.layer1[k] for k in range(4)])
    backbone.layer2, backbone.layer3, backbone.layer4 = StockStage(rx.layer2), StockStage(rx.layer3), StockStage(rx.layer4)
    return backbone


def stock_maps(backbone, x):
    maps = []
    for k in (1, 2, 3, 4):
        x = getattr(backbone, f"layer{k}")(x)
        maps.append(x)
    return maps


def seed_parameters(rx):
    gen = torch.Generator().manual_seed(32000)
    for c in TABLE:
        conv, bn = rx.get_submodule(c.key), rx.get_submodule(c.norm_key)
        bound = (6.0 / (conv.weight.shape[1] * c.kernel_size ** 2)) ** 0.5
        conv.weight.data.uniform_(-bound, bound, generator=gen)
        lo, hi = (0.2, 0.5) if c.name.endswith("conv3") else (0.5, 1.5)
        bn.weight.data.uniform_(lo, hi, generator=gen)
        bn.bias.data.normal_(0.0, 0.1, generator=gen)
        bn.running_mean.normal_(0.0, 0.1, generator=gen)
        bn.running_var.uniform_(0.5, 1.5, generator=gen)


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


def alternate(ours, theirs):
    rounds = {"module": [], "torch": []}
    for _ in range(args.rounds):
        rounds["module"].append(event_ms(ours, args.calls, warmup=2)["ms_median"])
        rounds["torch"].append(event_ms(theirs, args.calls, warmup=2)["ms_median"])
    entry = {"rounds": args.rounds, "calls_per_round": args.calls, "module_ms": rounds["module"], "torch_ms": rounds["torch"]}
    for k in ("module", "torch"):
        t = np.array(rounds[k])
        entry.update({f"{k}_ms_median": float(np.median(t)), f"{k}_ms_min": float(t.min()), f"{k}_ms_max": float(t.max())})
    entry["torch_over_module"] = entry["torch_ms_median"] / entry["module_ms_median"]
    return entry


result = {"shape": {"height": H, "width": W, "blocks": BLOCKS, "groups": GROUPS, "width_per_group": WIDTH_PER_GROUP,
                    "convolutions": len(TABLE)}, "f32_peak_tflops": PEAK / 1e12, "batches": {}}
with torch.no_grad():
    rx = midas.resnext101_32x8d()
    seed_parameters(rx)
    torch.manual_seed(32001)
    net = midas.MidasNet(backbone=rx).to(dev).eval()
    rx = net.pretrained
    stock = stock_backbone_of(rx)
    parent = midas.MidasNet(backbone=stock)
    parent.scratch = net.scratch                     # the same decoder parameters
    parent = parent.to(dev).eval()
    handle = tc.solver(dev)
    n = len(TABLE)
    w_table = (C.c_void_p * n)(*[rx.get_submodule(c.key).weight.data_ptr() for c in TABLE])
    n_table = (C.c_void_p * (4 * n))(*[t.data_ptr() for c in TABLE for t in midas._norm_vectors(rx.get_submodule(c.norm_key))])

    for batch in args.batches:
        images = torch.randn(batch, 3, H, W, device=dev)
        for _ in range(5):          # the vendor library's algorithm search, outside every timing
            parent(images)
            net(images)
        torch.cuda.synchronize(dev)
        ours, theirs = rx(images), stock_maps(stock, images)
        out_ours, out_theirs = net(images), parent(images)
        checks = {"maps_max_abs_diff_to_stock_torch": [float((a - b).abs().max()) for a, b in zip(ours, theirs)],
                  "maps_scale": [float(b.abs().max()) for b in theirs], "maps_zero_share": [float((b == 0).float().mean()) for b in theirs],
                  "net_max_abs_diff_to_parent_form": float((out_ours - out_theirs).abs().max()), "net_output_scale": float(out_theirs.abs().max()),
                  "repeat_equal": bool(all(torch.equal(a, b) for a, b in zip(rx(images), ours)))}
        print(f"B = {batch}: against the torch baseline:", checks, flush=True)
        assert checks["repeat_equal"] and all(d < 1e-3 * max(s, 1.0) for d, s in zip(checks["maps_max_abs_diff_to_stock_torch"], checks["maps_scale"]))
        entry = {"checks": checks}

        outs = [torch.empty_like(t) for t in ours]
        o_table = (C.c_void_p * 4)(*[t.data_ptr() for t in outs])
        ms = (C.c_double * (2 * n + 1))()

        def timed():
            stream = torch.cuda.current_stream(dev).cuda_stream
            handle._check(handle._fn("midas_backbone_timed")(
                handle._h, C.c_int32(batch), C.c_int32(H), C.c_int32(W), (C.c_int32 * 4)(*BLOCKS), C.c_int32(GROUPS), C.c_int32(WIDTH_PER_GROUP),
                C.c_float(api.RESNEXT_EPS), C.c_void_p(images.data_ptr()), w_table, n_table, o_table, C.c_void_p(stream), ms))
            return list(ms)
        for _ in range(3):
            timed()
        per_launch = np.array([timed() for _ in range(args.calls)])
        launches, kinds = {}, {}
        for i, c in enumerate(TABLE):
            hin, win, ho, wo = SIZES[i]
            launches[c.name] = dict(with_rate(stats(per_launch[:, 2 * i], args.calls), conv_flop(i, batch)), input=[hin, win],
                                    split=1 if c.groups > 1 else api.resnext_split(c.in_channels * c.kernel_size ** 2, ho * wo, c.kernel_size))
            if per_launch[:, 2 * i + 1].max() > 0:
                launches[c.name + ":fold"] = stats(per_launch[:, 2 * i + 1], args.calls)
            kind = "stem" if i == 0 else f"layer{c.name[5]}." + c.name.split(".", 2)[2]
            kinds.setdefault(kind, []).append(i)
        launches["maxpool"] = stats(per_launch[:, 2 * n], args.calls)
        entry["launches"] = launches
        # per stage and member (conv1, conv2 = the grouped 3 x 3, conv3, downsample.0): summed over the stage's blocks, folds included
        entry["by_kind"] = {k: with_rate(stats(sum(per_launch[:, 2 * i] + per_launch[:, 2 * i + 1] for i in idx), args.calls),
                                         sum(conv_flop(i, batch) for i in idx)) for k, idx in kinds.items()}
        total_flop = sum(conv_flop(i, batch) for i in range(n))
        entry["sum_of_launches"] = with_rate(stats(per_launch.sum(axis=1), args.calls), total_flop)
        entry["folds_ms_median"] = float(np.median(per_launch[:, 1:2 * n:2].sum(axis=1)))
        entry["launch_count"] = int((per_launch[0] > 0).sum())

        entry["backbone_call"] = dict(alternate(lambda: rx(images), lambda: stock_maps(stock, images)), gflop=total_flop / 1e9)
        entry["net_call"] = alternate(lambda: net(images), lambda: parent(images))
        result["batches"][str(batch)] = entry

    result["conditions"] = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
                            "timer": "HIP events",
                            "baseline": "the same backbone as stock torch modules (nn.Conv2d(groups=32), nn.BatchNorm2d.eval(), nn.MaxPool2d) "
                                        "on the same weight tensors, measured in the same run in alternating rounds",
                            "not_verified": "the trained checkpoint midas_v21-f6b98070.pt: weights are seeded He-scaled draws",
                            "not_profiled": "no counters, no per-kernel trace of the torch baseline"}

for batch, entry in result["batches"].items():
    for k, v in entry["by_kind"].items():
        print(f"B = {batch} {k}: {v['ms_median']:.3f} ms ({v['ms_min']:.3f} .. {v['ms_max']:.3f}); {v['gflop']:.2f} GFLOP -> "
              f"{v.get('tflops', 0.0):.1f} TF = {100 * v.get('share_of_157tf', 0.0):.1f} % of 157 TF", flush=True)
    for label, key in (("backbone", "backbone_call"), ("MidasNet", "net_call")):
        c = entry[key]
        print(f"B = {batch} {label}: module {c['module_ms_median']:.3f} ms ({c['module_ms_min']:.3f} .. {c['module_ms_max']:.3f}); stock torch "
              f"{c['torch_ms_median']:.3f} ms ({c['torch_ms_min']:.3f} .. {c['torch_ms_max']:.3f}); torch / module = {c['torch_over_module']:.2f} "
              f"(medians of {c['rounds']} alternating rounds)", flush=True)
    s = entry["sum_of_launches"]
    print(f"B = {batch}: {entry['launch_count']} launches sum to {s['ms_median']:.3f} ms ({s['ms_min']:.3f} .. {s['ms_max']:.3f}), folds "
          f"{entry['folds_ms_median']:.3f} ms; maxpool {entry['launches']['maxpool']['ms_median']:.3f} ms", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
