"""Development aid (GPU): training the MiDaS v2.1 backbone (csrc/cvd_resnext_grad.h, robust_cvd_amd.midas_train.ResNeXt, DESIGN.md
§3.22) at 384 x 224, B = 1 and 8.  HIP-event medians with min .. max:

  operators   every operator kind of a stage's repeated block (norm forward / backward, grouped input / weight gradient, conv3's
              1 x 1 input / weight gradient), the stem's weight gradient and the pool's backward, with GFLOP and the share of the
              157 TF f32 peak where the operator has flops
  backbone    forward + backward of midas_train.ResNeXt against the same backbone in stock torch ops under autograd, both in
              training mode, in alternating rounds
  step        a whole MidasNet training step (forward, backward) against the parent's best form: the stock backbone under autograd
              in front of the native decoder
  saved       the bytes the backbone's training forward keeps per frame (api.resnext_saved_bytes)

    python tools/midasnet_grad_bench.py --out profiles/midasnet_grad_bench.json [--rounds 5] [--batches 1 8]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robust_cvd_amd import api, midas, midas_train  # noqa: E402
from robust_cvd_amd import torch_common as tc       # noqa: E402
from tests import resnext_reference as rr           # noqa: E402

DEV = torch.device("cuda", 0)
PEAK_TF = 157.0
H, W = 224, 384
_i32 = C.c_int32


def timed(fn, rounds, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def with_flops(t, gflop):
    t["gflop"] = gflop
    t["share_of_f32_peak"] = gflop / t["median_ms"] / PEAK_TF if gflop else None
    return t


def rand(*shape):
    return torch.randn(*shape, device=DEV)


def operators(B, rounds):
    out = {}
    call = lambda name, *args: midas._call(DEV, name, *args)
    p = tc.ptr
    for k in range(4):
        planes, h, w = 64 << k, H >> (k + 2), W >> (k + 2)
        width, outc, cg = planes * 8 // 64 * 32, 4 * planes, planes * 8 // 64
        M = B * h * w
        c, y, gy, gc = rand(B, width, h, w), rand(B, width, h, w), rand(B, width, h, w), torch.empty(B, width, h, w, device=DEV)
        vec = [torch.rand(width, device=DEV) + 0.5 for _ in range(6)]
        gg, gb = torch.empty(width, device=DEV), torch.empty(width, device=DEV)
        dims = (_i32(B), _i32(width), _i32(h), _i32(w))
        stage = {}
        stage["norm_train"] = timed(lambda: call("resnext_norm_train_device", *dims, p(c), p(vec[0]), p(vec[1]), p(vec[2]), p(vec[3]),
                                                 C.c_double(1e-5), C.c_double(0.1), _i32(1), _i32(1), None, p(vec[4]), p(vec[5]), p(y)), rounds)
        stage["norm_grad"] = timed(lambda: call("resnext_norm_grad_device", *dims, p(gy), p(c), p(y), p(vec[4]), p(vec[5]), p(vec[0]),
                                                _i32(1), p(gc), p(gg), p(gb), None), rounds)
        wg, gwg = rand(width, cg, 3, 3), torch.empty(width, cg, 3, 3, device=DEV)
        gdims = (_i32(B), _i32(h), _i32(w), _i32(32), _i32(cg), _i32(1))
        gflop = 2.0 * M * width * cg * 9 / 1e9
        stage["grouped_grad_input"] = with_flops(timed(lambda: call("resnext_grouped_conv_grad_input_device", *gdims, p(gy), p(wg), p(gc)),
                                                       rounds), gflop)
        stage["grouped_grad_weight"] = with_flops(timed(lambda: call("resnext_grouped_conv_grad_weight_device", *gdims, p(gy), p(c),
                                                                     _i32(0), p(gwg)), rounds), gflop)
        g3, w3, gw3 = rand(B, outc, h, w), rand(outc, width, 1, 1), torch.empty(outc, width, 1, 1, device=DEV)
        ddims = (_i32(B), _i32(h), _i32(w), _i32(width), _i32(outc), _i32(1), _i32(1))
        gflop = 2.0 * M * width * outc / 1e9
        stage["conv3_grad_input"] = with_flops(timed(lambda: call("resnext_conv_grad_input_device", *ddims, p(g3), p(w3), None, p(gc)),
                                                     rounds), gflop)
        stage["conv3_grad_weight"] = with_flops(timed(lambda: call("resnext_conv_grad_weight_device", *ddims, p(g3), p(c), _i32(0),
                                                                   p(gw3)), rounds), gflop)
        out[f"layer{k + 1}"] = stage
    x, gs, gw = rand(B, 3, H, W), rand(B, 64, H // 2, W // 2), torch.empty(64, 3, 7, 7, device=DEV)
    out["stem_grad_weight"] = with_flops(timed(lambda: call("resnext_conv_grad_weight_device", _i32(B), _i32(H), _i32(W), _i32(3), _i32(64),
                                                            _i32(7), _i32(2), p(gs), p(x), _i32(0), p(gw)), rounds),
                                         2.0 * B * (H // 2) * (W // 2) * 64 * 147 / 1e9)
    gp, gxs = rand(B, 64, H // 4, W // 4), torch.empty(B, 64, H // 2, W // 2, device=DEV)
    out["maxpool_grad"] = timed(lambda: call("resnext_maxpool_grad_device", _i32(B), _i32(64), _i32(H // 2), _i32(W // 2), p(gs), p(gp),
                                             p(gxs)), rounds)
    return out


def stock_backbone():
    return rr.midas_backbone(rr.stock_resnet(*api.RESNEXT101_32X8D))


def backbone_step(net, x):
    def run():
        for q in net.parameters():
            q.grad = None
        maps, t = [], x
        for k in (1, 2, 3, 4):
            t = getattr(net, f"layer{k}")(t)
            maps.append(t)
        sum(m.sum() for m in maps).backward()
    return run


def net_step(net, x):
    def run():
        for q in net.parameters():
            q.grad = None
        net(x).sum().backward()
    return run


def alternate(pairs, rounds):
    """{name: times} of the callables, one timed call each per round, in alternating order."""
    ms = {n: [] for n in pairs}
    for fn in pairs.values():
        fn()
    for _ in range(rounds):
        for n, fn in pairs.items():
            ms[n].append(timed(fn, 1, warm=0)["median_ms"])
    return {n: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for n, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    args = ap.parse_args()
    torch.manual_seed(0)
    result = {"shape": [H, W], "f32_peak_tflops": PEAK_TF, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
              "saved_bytes_per_frame": api.resnext_saved_bytes(H, W), "batches": {}}
    native = midas_train.resnext101_32x8d().to(DEV).train()
    stock = stock_backbone().to(DEV).train()
    full_native = midas_train.MidasNet(backbone=midas_train.resnext101_32x8d(), non_negative=False).to(DEV).train()
    full_stock = midas_train.MidasNet(backbone=stock_backbone(), non_negative=False).to(DEV).train()
    for B in args.batches:
        x = rand(B, 3, H, W)
        entry = {"operators": operators(B, args.rounds)}
        entry["backbone_forward_backward"] = alternate({"native": backbone_step(native, x), "stock_torch": backbone_step(stock, x)},
                                                       args.rounds)
        entry["training_step_forward_backward"] = alternate({"native": net_step(full_native, x),
                                                             "stock_backbone_native_decoder": net_step(full_stock, x)}, args.rounds)
        result["batches"][str(B)] = entry
        print(json.dumps({"B": B, "backbone": entry["backbone_forward_backward"], "step": entry["training_step_forward_backward"]}), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
