"""Development aid (GPU): RAFT's feature and context encoders (csrc/cvd_raftenc.h, robust_cvd_amd.raft_ops.BasicEncoder) and one
directed flow pair end to end through robust_cvd_amd.raft_ops.RAFT, at the flow stage's working size: B = 1, 576 x 1024 images.

Kernel times are HIP-event times (median of --calls after warm-up, with min .. max): every launch of both encoders through the
library's timed entry point (fnet on the pair, B = 2, instance norm; cnet, B = 1, batch norm), each encoder's whole call through
the module on torch's current stream against the stock-torch encoder with the same weights (Conv2d, InstanceNorm2d / BatchNorm2d in
eval mode, ReLU as raft/core/extractor.py writes them; warmed up so that the vendor library's algorithm search lies outside the
timing).  FLOP = 2 M K N per convolution; the share of the 157 TF f32 matrix peak is what the times imply.  The pair figure is
RAFT.forward(iters=20, test_mode=True) against the parent commit's best form: the stock-torch encoders around the project's
CorrBlock, BasicUpdateBlock and upsample_flow, every iteration's mask and upsampling computed as the reference's loop does; rounds
alternate in one process.  Seeded random inputs (never zeros).
Usage: python tools/raftenc_bench.py [--out profiles/raftenc_bench.json] [--calls 20] [--height 576 --width 1024]"""
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
from robust_cvd_amd.raft_ops import RAFT, CorrBlock, upsample_flow

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--height", type=int, default=576)
ap.add_argument("--width", type=int, default=1024)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("raftenc_bench needs a GPU: there is nothing to measure without one")
dev = torch.device("cuda", 0)
H, W = args.height, args.width
PEAK = 157e12


def layer_flops(batch):
    """FLOP of the sixteen convolutions for `batch` images, in the entry point's order."""
    size = {1: (api.raft_encoder_out_size(H, 2), api.raft_encoder_out_size(W, 2)),
            2: (api.raft_encoder_out_size(H, 4), api.raft_encoder_out_size(W, 4)),
            3: (api.raft_encoder_out_size(H, 8), api.raft_encoder_out_size(W, 8))}
    out = []
    for name, o, c, k, _s in api.ENCODER_LAYERS:
        level = 1 if name == "conv1" else 3 if name == "conv2" else int(name[5])
        h, w = size[level]
        out.append(2.0 * batch * h * w * c * k * k * (256 if o is None else o))
    return out


class StockEncoder(torch.nn.Module):
    """BasicEncoder with stock torch modules under the reference's names (raft/core/extractor.py:124-197 restated)."""

    class Block(torch.nn.Module):
        def __init__(self, cin, planes, norm, stride):
            super().__init__()
            self.conv1 = torch.nn.Conv2d(cin, planes, 3, padding=1, stride=stride)
            self.conv2 = torch.nn.Conv2d(planes, planes, 3, padding=1)
            self.norm1, self.norm2 = norm(planes), norm(planes)
            self.downsample = None
            if stride != 1:
                self.norm3 = norm(planes)
                self.downsample = torch.nn.Sequential(torch.nn.Conv2d(cin, planes, 1, stride=stride), self.norm3)

        def forward(self, x):
            y = F.relu(self.norm1(self.conv1(x)))
            y = F.relu(self.norm2(self.conv2(y)))
            if self.downsample is not None:
                x = self.downsample(x)
            return F.relu(x + y)

    def __init__(self, output_dim, norm_fn):
        super().__init__()
        norm = torch.nn.InstanceNorm2d if norm_fn == "instance" else torch.nn.BatchNorm2d
        self.norm1 = norm(64)
        self.conv1 = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3)
        self.layer1 = torch.nn.Sequential(self.Block(64, 64, norm, 1), self.Block(64, 64, norm, 1))
        self.layer2 = torch.nn.Sequential(self.Block(64, 96, norm, 2), self.Block(96, 96, norm, 1))
        self.layer3 = torch.nn.Sequential(self.Block(96, 128, norm, 2), self.Block(128, 128, norm, 1))
        self.conv2 = torch.nn.Conv2d(128, output_dim, 1)

    def forward(self, x):
        is_list = isinstance(x, (tuple, list))
        if is_list:
            batch = x[0].shape[0]
            x = torch.cat(x, dim=0)
        x = F.relu(self.norm1(self.conv1(x)))
        x = self.conv2(self.layer3(self.layer2(self.layer1(x))))
        return torch.split(x, [batch, batch], dim=0) if is_list else x


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


torch.manual_seed(31800)
with torch.no_grad():
    model = RAFT(argparse.Namespace(small=False, mixed_precision=False)).to(dev).eval()
    # non-trivial running statistics, as a trained checkpoint has
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0.0, 0.5)
            m.running_var.uniform_(0.5, 2.0)
            m.weight.uniform_(0.5, 1.5)
            m.bias.normal_(0.0, 0.3)
    stock_f, stock_c = StockEncoder(256, "instance").to(dev).eval(), StockEncoder(256, "batch").to(dev).eval()
    stock_f.load_state_dict(model.fnet.state_dict())
    stock_c.load_state_dict(model.cnet.state_dict())
    image1 = torch.rand(1, 3, H, W, device=dev) * 255.0
    image2 = torch.roll(image1, 3, dims=3) + torch.randn(1, 3, H, W, device=dev)
    x1, x2 = (2 * (image1 / 255.0) - 1.0).contiguous(), (2 * (image2 / 255.0) - 1.0).contiguous()

    for _ in range(5):          # the vendor library's algorithm search, outside every timing
        stock_f([x1, x2])
        stock_c(x1)
    torch.cuda.synchronize(dev)
    f_ours, f_stock = model.fnet([x1, x2]), stock_f([x1, x2])
    checks = {"fnet_max_abs_diff_to_stock_torch": max(float((a - b).abs().max()) for a, b in zip(f_ours, f_stock)),
              "cnet_max_abs_diff_to_stock_torch": float((model.cnet(x1) - stock_c(x1)).abs().max()),
              "repeat_equal": bool(torch.equal(model.fnet([x1, x2])[0], f_ours[0]) and torch.equal(model.cnet(x1), model.cnet(x1)))}
    print("modules against the torch baseline:", checks, flush=True)
    assert max(checks["fnet_max_abs_diff_to_stock_torch"], checks["cnet_max_abs_diff_to_stock_torch"]) < 1e-3 and checks["repeat_equal"]

    result = {"shape": {"height": H, "width": W, "features": [H // 8, W // 8]}, "checks": checks, "f32_matrix_peak_tflops": PEAK / 1e12}

    # every launch, through the timed entry point (events around each launch on torch's stream, a host wait)
    handle = tc.solver(dev)

    def timed_encoder(module, x, mode):
        convs = [module.get_submodule(n) for n in api.ENCODER_PARAMETERS]
        w_table = (C.c_void_p * 16)(*[m.weight.data_ptr() for m in convs])
        b_table = (C.c_void_p * 16)(*[m.bias.data_ptr() for m in convs])
        n_table = None
        if mode == 2:
            vectors = [getattr(module.get_submodule(n), v) for n in api.ENCODER_NORMS for v in api.ENCODER_NORM_VECTORS]
            n_table = (C.c_void_p * 60)(*[t.data_ptr() for t in vectors])
        batch = x.shape[0]
        out = torch.empty(batch, 256, H // 8, W // 8, device=dev)
        ms = (C.c_double * 48)()

        def timed():
            stream = torch.cuda.current_stream(dev).cuda_stream
            handle._check(handle._fn("raft_encoder_timed")(
                handle._h, C.c_int32(batch), C.c_int32(H), C.c_int32(W), C.c_int32(256), C.c_int32(mode), C.c_float(1e-5),
                C.c_void_p(x.data_ptr()), w_table, b_table, n_table, C.c_void_p(out.data_ptr()), C.c_void_p(stream), ms))
            return list(ms)
        for _ in range(3):
            timed()
        per_launch = np.array([timed() for _ in range(args.calls)])
        flops = layer_flops(batch)
        launches = {}
        for i, name in enumerate(api.ENCODER_PARAMETERS):
            launches[name] = with_rate(stats(per_launch[:, 3 * i], args.calls), flops[i])
            if mode == 1 and i < 15:
                launches[name + ":norm_stats"] = stats(per_launch[:, 3 * i + 1], args.calls)
                launches[name + ":norm_apply"] = stats(per_launch[:, 3 * i + 2], args.calls)
        total = per_launch.sum(axis=1)
        return {"launches": launches, "sum_of_launches": with_rate(stats(total, args.calls), sum(flops)),
                "convolutions_ms_median": float(np.median(per_launch[:, 0::3].sum(axis=1))),
                "norm_stats_ms_median": float(np.median(per_launch[:, 1::3].sum(axis=1))),
                "norm_apply_ms_median": float(np.median(per_launch[:, 2::3].sum(axis=1)))}

    pair = torch.cat([x1, x2], 0).contiguous()
    result["fnet"] = timed_encoder(model.fnet, pair, 1)
    result["cnet"] = timed_encoder(model.cnet, x1, 2)
    result["fnet"]["call"] = with_rate(event_ms(lambda: model.fnet([x1, x2]), args.calls), sum(layer_flops(2)))
    result["fnet"]["call_torch"] = with_rate(event_ms(lambda: stock_f([x1, x2]), args.calls), sum(layer_flops(2)))
    result["cnet"]["call"] = with_rate(event_ms(lambda: model.cnet(x1), args.calls), sum(layer_flops(1)))
    result["cnet"]["call_torch"] = with_rate(event_ms(lambda: stock_c(x1), args.calls), sum(layer_flops(1)))

    # one directed pair end to end: the module against the parent commit's best form
    def parent_form(image1, image2):
        a = (2 * (image1 / 255.0) - 1.0).contiguous()
        b = (2 * (image2 / 255.0) - 1.0).contiguous()
        fmap1, fmap2 = stock_f([a, b])
        corr_fn = CorrBlock(fmap1.contiguous(), fmap2.contiguous(), radius=4)
        net, inp = torch.split(stock_c(a), [128, 128], dim=1)
        net, inp = torch.tanh(net), torch.relu(inp)
        h, w = H // 8, W // 8
        ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
        coords0 = torch.stack([xs, ys], dim=0).float()[None]
        coords1 = coords0.clone()
        for _ in range(args.iters):
            net, mask, delta = model.update_block(net, inp, corr_fn(coords1), coords1 - coords0)
            coords1 = coords1 + delta
            up = upsample_flow(coords1 - coords0, mask)
        return coords1 - coords0, up

    ours = lambda: model(image1, image2, iters=args.iters, test_mode=True)  # noqa: E731
    pair_diff = float((ours()[1] - parent_form(image1, image2)[1]).abs().max())
    rounds = {"module": [], "parent": []}
    for _ in range(args.rounds):                                   # alternating rounds in one process
        rounds["module"].append(event_ms(ours, 1, warmup=1)["ms_median"])
        rounds["parent"].append(event_ms(lambda: parent_form(image1, image2), 1, warmup=1)["ms_median"])
    result["pair"] = {"iterations": args.iters, "rounds": args.rounds, "max_abs_diff_flow_up": pair_diff,
                      "module_ms": rounds["module"], "parent_ms": rounds["parent"]}
    for k in ("module", "parent"):
        t = np.array(rounds[k])
        result["pair"].update({f"{k}_ms_median": float(np.median(t)), f"{k}_ms_min": float(t.min()), f"{k}_ms_max": float(t.max())})
    result["pair"]["speedup"] = result["pair"]["parent_ms_median"] / result["pair"]["module_ms_median"]
    result["conditions"] = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
                            "timer": "HIP events", "not_profiled": "no counters, no per-kernel trace of the torch baseline"}

for enc in ("fnet", "cnet"):
    for n, k in result[enc]["launches"].items():
        rate = f"; {k['gflop']:.2f} GFLOP -> {k['tflops']:.1f} TF = {100 * k['share_of_157tf']:.1f} % of 157 TF" if "tflops" in k else ""
        print(f"{enc} {n}: {k['ms_median']:.3f} ms (median of {k['calls']}, {k['ms_min']:.3f} .. {k['ms_max']:.3f}){rate}", flush=True)
    r = result[enc]
    c, t = r["call"], r["call_torch"]
    print(f"{enc}: launches {r['sum_of_launches']['ms_median']:.3f} ms (convolutions {r['convolutions_ms_median']:.3f}, norm statistics "
          f"{r['norm_stats_ms_median']:.3f}, norm elementwise {r['norm_apply_ms_median']:.3f}); call {c['ms_median']:.3f} ms "
          f"({c['ms_min']:.3f} .. {c['ms_max']:.3f}; {c['tflops']:.1f} TF); stock torch {t['ms_median']:.3f} ms ({t['ms_min']:.3f} .. "
          f"{t['ms_max']:.3f}; {t['tflops']:.1f} TF)", flush=True)
p = result["pair"]
print(f"pair, {p['iterations']} iterations: module {p['module_ms_median']:.2f} ms ({p['module_ms_min']:.2f} .. {p['module_ms_max']:.2f}), "
      f"parent form {p['parent_ms_median']:.2f} ms ({p['parent_ms_min']:.2f} .. {p['parent_ms_max']:.2f}) (x {p['speedup']:.2f}; medians of "
      f"{p['rounds']} alternating rounds; flow_up differs by {p['max_abs_diff_flow_up']:.2e})", flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
print(json.dumps(result))
