"""Development aid (GPU): the backward of the MiDaS v2.1 decoder (csrc/cvd_midas_grad.h, robust_cvd_amd.midas_train.MidasNet) at the
depth stage's working size: 384 x 224 frames (feature maps 96 x 56 down to 12 x 7), B = 1 and B = 8, features = 256.

Times are HIP-event times (median of --calls after warm-up, with min .. max): per distinct layer shape of the decoder the weight
gradient and the input gradient through midas_train's operator calls on torch's current stream (a call is one to three launches:
transform or convolution, fold, bias), with the GEMM's GFLOP (2 M K N; the rate and the share of the 157 TF f32 matrix peak are per
CALL) and the weight gradient's split; the head's backward; every operator call of the one-call decoder backward through
cvd_midas_decoder_backward_timed; at B > 1 the batch's map gradients against its images one by one; and forward +
backward of midas_train.MidasNet.decode (parameter gradients and the four feature-map gradients) against a stock-torch decoder with
the same weights under torch's autograd (tools/midas_bench.py's, the reference's in-place ReLU semantics), in alternating rounds in
one process, warmed up so that the vendor library's algorithm search lies outside the timing.  Also max |native - stock-torch
gradient| / max |gradient| per parameter tensor at that shape.  Seeded random inputs (never zeros).  The backbone is not part of any
figure: the feature maps are inputs.
Usage: python tools/midas_grad_bench.py [--out profiles/midas_grad_bench.json] [--calls 10] [--rounds 3]"""
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
from robust_cvd_amd import midas_train
from robust_cvd_amd import torch_common as tc

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--height", type=int, default=224)
ap.add_argument("--width", type=int, default=384)
ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("midas_grad_bench needs a GPU: there is nothing to measure without one")
if args.height % 32 or args.width % 32:
    sys.exit("height and width must be multiples of 32")
dev = torch.device("cuda", 0)
H, W = args.height, args.width
PEAK = 157e12
FEATURES = 256
CHANNELS = api.MIDAS_BACKBONE_CHANNELS
SIZES = [(H >> (k + 2), W >> (k + 2)) for k in range(4)]


def stock_unit(x, unit):
    r = F.relu(x)
    return F.conv2d(F.relu(F.conv2d(r, unit.conv1.weight, unit.conv1.bias, padding=1)), unit.conv2.weight, unit.conv2.bias, padding=1) + r


def stock_decoder(net, maps):
    s = net.scratch
    rn = [F.conv2d(m, getattr(s, f"layer{k + 1}_rn").weight, None, padding=1) for k, m in enumerate(maps)]
    path = None
    for k in (4, 3, 2, 1):
        block = getattr(s, f"refinenet{k}")
        out = rn[k - 1]
        if path is not None:
            out = path + stock_unit(out, block.resConfUnit1)
        path = F.interpolate(stock_unit(out, block.resConfUnit2), scale_factor=2, mode="bilinear", align_corners=True)
    oc = s.output_conv
    y = F.interpolate(F.conv2d(path, oc[0].weight, oc[0].bias, padding=1), scale_factor=2, mode="bilinear", align_corners=False)
    y = F.conv2d(F.relu(F.conv2d(y, oc[2].weight, oc[2].bias, padding=1)), oc[4].weight, oc[4].bias)
    return F.relu(y).squeeze(1)


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


torch.manual_seed(32100)
result = {"shape": {"height": H, "width": W, "features": FEATURES, "feature_maps": SIZES}, "f32_matrix_peak_tflops": PEAK / 1e12, "batches": {}}
backbone = torch.nn.Module()          # never run: the feature maps are the inputs here
for k in (1, 2, 3, 4):
    setattr(backbone, f"layer{k}", torch.nn.Identity())
net = midas_train.MidasNet(features=FEATURES, backbone=backbone).to(dev).train()
with torch.no_grad():
    net.scratch.output_conv[4].bias.fill_(0.5)

# the decoder's distinct layer shapes: (label, in, out, (h, w), how often it runs, input gradient needed)
half = (2 * SIZES[0][0], 2 * SIZES[0][1])
LAYERS = [(f"layer{k + 1}_rn", CHANNELS[k], FEATURES, SIZES[k], 1) for k in range(4)]
LAYERS += [(f"refinenet{k + 1} unit convolution", FEATURES, FEATURES, SIZES[k], 2 if k == 3 else 4) for k in range(4)]
LAYERS += [("output_conv.0", FEATURES, 128, half, 1), ("output_conv.2", 128, 32, (H, W), 1)]

for batch in args.batches:
    entry = {}
    operators = {}
    for label, cin, cout, (h, w), count in LAYERS:
        gy = torch.randn(batch, cout, h, w, device=dev)
        x = torch.randn(batch, cin, h, w, device=dev)
        weight = torch.randn(cout, cin, 3, 3, device=dev) / (3.0 * cin ** 0.5)
        flop = 2.0 * batch * h * w * cin * 9 * cout
        operators[label] = {
            "runs_per_backward": count, "pixels": batch * h * w,
            "weight_gradient": dict(with_rate(event_ms(lambda: midas_train._grad_weight(gy, x, 3, True, True), args.calls), flop),
                                    split=api.midas_wgrad_split(batch * h * w, cout, cin * 9)),
            # (as the decoder runs it: the unit convolutions masked -- the folded path --, layerK_rn and output_conv.0 not)
            "input_gradient": dict(with_rate(event_ms(lambda: midas_train._grad_input(gy, weight, add=None, mask=x if "unit" in label or label == "output_conv.2" else None),
                                                      args.calls), flop),
                                   split=api.midas_split(cout * 9, h * w))}
        print(f"B = {batch} {label}: wgrad {operators[label]['weight_gradient']['ms_median']:.3f} ms, "
              f"dgrad {operators[label]['input_gradient']['ms_median']:.3f} ms", flush=True)
    # the head's backward: the recomputed pre-activation and output, the pointwise kernel, output_conv.2's two gradients
    oc = net.scratch.output_conv
    tensors = [torch.randn(batch, 128, H, W, device=dev)] + [t.detach().contiguous() for t in (oc[2].weight, oc[2].bias, oc[4].weight, oc[4].bias)]
    gy = torch.randn(batch, H, W, device=dev)
    grads = [torch.empty_like(t) for t in tensors]
    i32 = midas_train._i32
    head_flop = 3 * 2.0 * batch * H * W * 128 * 9 * 32          # the recomputed convolution and its two gradients
    operators["head"] = with_rate(event_ms(lambda: midas._call(
        dev, "midas_head_grad_device", i32(batch), i32(H), i32(W), i32(128), i32(32), tc.ptr(gy), *[tc.ptr(t) for t in tensors], i32(1),
        *[tc.ptr(g) for g in grads]), args.calls), head_flop)
    print(f"B = {batch} head backward: {operators['head']['ms_median']:.3f} ms", flush=True)
    entry["operators"] = operators

    maps = [torch.relu(torch.randn(batch, c, h, w, device=dev)).contiguous().requires_grad_(True) for c, (h, w) in zip(CHANNELS, SIZES)]
    wsum = torch.randn(batch, H, W, device=dev)

    def run(decoder):
        net.zero_grad(set_to_none=True)
        for m in maps:
            m.grad = None
        (decoder(*maps) * wsum).sum().backward()

    native = lambda *m: net.decode(*m)
    stock = lambda *m: stock_decoder(net, m)
    for _ in range(3):          # the vendor library's algorithm search, outside every timing
        run(stock)
    run(native)
    torch.cuda.synchronize(dev)
    ours = {n: p.grad.clone() for n, p in net.scratch.named_parameters() if p.grad is not None}
    ours.update({f"layer_{k + 1}": m.grad.clone() for k, m in enumerate(maps)})
    run(stock)
    theirs = {n: p.grad.clone() for n, p in net.scratch.named_parameters() if p.grad is not None}
    theirs.update({f"layer_{k + 1}": m.grad.clone() for k, m in enumerate(maps)})
    assert sorted(ours) == sorted(theirs) and len(ours) == 38 + 4
    entry["gradient_max_abs_diff_over_scale"] = {n: float((ours[n] - theirs[n]).abs().max() / theirs[n].abs().max()) for n in ours}
    worst = max(entry["gradient_max_abs_diff_over_scale"].values())
    print(f"B = {batch}: worst max |native - stock torch| / max |gradient| over 42 tensors: {worst:.3e}", flush=True)
    assert worst < 0.5, "a gradient far from stock torch's"          # (a sanity check: ties at the ReLUs may differ between the two)

    # the one-call backward, stage by stage: HIP events around every operator call cvd_midas_decoder_backward_timed makes (each one to
    # three launches: transform or convolution, fold, bias), exactly the calls MidasNet.decode's backward makes
    plain = [m.detach() for m in maps]
    convs = [net.scratch.get_submodule(n) for n in api.MIDAS_PARAMETERS]
    weights, biases = [m.weight.detach() for m in convs], [m.bias.detach() for m in convs[4:]]
    dims = (i32(batch), i32(FEATURES), (i32 * 4)(*CHANNELS), (i32 * 4)(*[sz[0] for sz in SIZES]), (i32 * 4)(*[sz[1] for sz in SIZES]))
    saved = [torch.empty(sh, device=dev) for sh in api.midas_saved_shapes(batch, FEATURES, [sz[0] for sz in SIZES], [sz[1] for sz in SIZES])]
    out = torch.empty(batch, H, W, device=dev)
    table = midas_train._table
    midas._call(dev, "midas_decoder_train_device", *dims, table(plain), table(weights), table(biases), i32(1), table(saved), tc.ptr(out))
    gws, gbs, gms = [torch.empty_like(t) for t in weights], [torch.empty_like(t) for t in biases], [torch.empty_like(t) for t in plain]
    ms = (C.c_double * api.MIDAS_BACKWARD_SLOTS)()

    def timed():
        handle = tc.solver(dev)
        handle._check(handle._fn("midas_decoder_backward_timed")(
            handle._h, *dims, tc.ptr(wsum), table(plain), table(saved), table(weights), table(biases), i32(1), table(gws), table(gbs),
            table(gms), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), ms))
        return list(ms)
    per_stage = np.array([timed() for _ in range(3 + args.calls)][3:])
    stage_names = api.midas_backward_stages(True)
    entry["backward_stages"] = {f"{i:02d} {n}": stats(per_stage[:, i], args.calls) for i, n in enumerate(stage_names)}
    entry["backward_sum_of_stages"] = stats(per_stage.sum(axis=1), args.calls)
    groups = {"weight gradients": ":wgrad", "input gradients": ":dgrad", "upsamplings": "upsample", "head": "head:"}
    entry["backward_ms_median_by_kind"] = {g: float(np.median(per_stage[:, [i for i, n in enumerate(stage_names) if key in n]].sum(axis=1)))
                                           for g, key in groups.items()}
    print(f"B = {batch}: one-call backward, sum of stages {entry['backward_sum_of_stages']['ms_median']:.2f} ms:", entry["backward_ms_median_by_kind"], flush=True)
    assert all(torch.equal(a, ours[f"layer_{k + 1}"]) for k, a in enumerate(gms)), "the timed call's map gradients differ from decode's"

    # at this size too: the map gradients of the batch are those of its images one by one, bit for bit
    if batch > 1:
        same = True
        for b in range(batch):
            leaves = [m.detach()[b:b + 1].clone().requires_grad_(True) for m in maps]
            net.zero_grad(set_to_none=True)
            (net.decode(*leaves) * wsum[b:b + 1]).sum().backward()
            same &= all(torch.equal(l.grad, ours[f"layer_{k + 1}"][b:b + 1]) for k, l in enumerate(leaves))
        entry["map_gradients_of_the_batch_equal_its_images_one_by_one"] = bool(same)
        print(f"B = {batch}: map gradients of the batch == images one by one: {same}", flush=True)
        assert same

    rounds = {"module": [], "torch": []}
    for _ in range(args.rounds):
        rounds["module"].append(event_ms(lambda: run(native), args.calls, warmup=2)["ms_median"])
        rounds["torch"].append(event_ms(lambda: run(stock), args.calls, warmup=2)["ms_median"])
    call = {"rounds": args.rounds, "calls_per_round": args.calls, "module_ms": rounds["module"], "torch_ms": rounds["torch"]}
    for k in ("module", "torch"):
        t = np.array(rounds[k])
        call.update({f"{k}_ms_median": float(np.median(t)), f"{k}_ms_min": float(t.min()), f"{k}_ms_max": float(t.max())})
    call["torch_over_module"] = call["torch_ms_median"] / call["module_ms_median"]
    entry["forward_backward"] = call
    print(f"B = {batch}: forward + backward module {call['module_ms_median']:.2f} ms, stock torch {call['torch_ms_median']:.2f} ms", flush=True)
    result["batches"][str(batch)] = entry

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)
