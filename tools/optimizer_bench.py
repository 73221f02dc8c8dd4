#!/usr/bin/env python3
"""Measure the fused parameter regulariser and optimizer step (robust_cvd_amd/csrc/cvd_paramstep.h) on the GPU
against what they replace, and sweep CVD_PARAM_CHUNK.

    python tools/optimizer_bench.py --build-variants          # no GPU needed: the sweep's libraries (cvd_frontend recompiled)
    python tools/optimizer_bench.py --out profiles/optimizer_bench.json

The parameter list is SYNTHETIC (the real depth network's shapes need weights that are not in this repository): 440 float32
tensors whose sizes are log-spaced between 64 and the largest that makes the total 105 M elements, in a seeded order; the first
output line describes it.  Every other line is one measurement:
  * kernel: the entry point called directly with prebuilt address tables, KERNEL_CALLS times back to back between two device
    events on torch's stream, the span divided by the number of calls.  The span holds the launches, the asynchronous table
    refresh of every call and whatever gap the enqueue leaves, so `median_ms` is an UPPER bound on the kernel's own time (the
    device runs behind the host within a window, which keeps the gaps small) and `gbps` / `hbm_share` LOWER bounds: `gbps` =
    algorithmic bytes (p, g, m, v read and p, m, v written: 28 B per element; moments only, which leaves p alone, 20; the loss
    8, its gradient 12) over that time, `hbm_share` = gbps over the 8 TB/s peak (about 6.3 TB/s is what a copy achieves: the
    bound of these kernels is bandwidth, not arithmetic);
  * wall: host clock around one call of the public surface (`step()`, or ParameterLoss plus backward) that ends in a device
    synchronise -- it includes the Python that builds the tables -- for this package and for what it replaces: torch.optim.Adam
    (foreach and fused=True), a per-tensor RAdam loop restated here from the reference's optimizer/radam.py, and the torch
    ParameterLoss of robust_cvd_amd/joint_loss.py;
  * sweep: the kernel lines of the step (Adam) and of the loss for each library variant built with another CVD_PARAM_CHUNK, each
    in a child process (a process loads one library).  The sweep stops at the first child that does not end with status 0 or
    runs out of time: nothing more is started on the GPU, the variants left are recorded as not measured, what was measured
    is written, and the tool exits with status 1.
Every figure is the median of --repeats calls after --warmup calls, with the minimum and maximum beside it.  There is no
pass / fail threshold on time.  Without a GPU the tool fails: nothing here is an estimate.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP = (8192, 65536, 262144)      # beside the product build's own constant
NUM_TENSORS, TOTAL, SMALLEST, SEED = 440, 105_000_000, 64, 4242
HBM_PEAK = 8.0e12
LAMBDA = 1e-3
KERNEL_CALLS = 10     # back-to-back entry-point calls per timed window of a kernel line


def variant_name(chunk):
    return f"chunk{chunk}"


def build_variants():
    from robust_cvd_amd import build
    for chunk in SWEEP:
        print(build.build_variant(variant_name(chunk), [f"CVD_PARAM_CHUNK={chunk}"], units=["cvd_frontend"], verbose=True))


def tensor_sizes():
    """NUM_TENSORS sizes, log-spaced from SMALLEST, that sum to about TOTAL, in a seeded order."""
    import numpy as np
    lo, hi = float(SMALLEST), float(TOTAL)
    for _ in range(200):       # bisection on the largest size
        mid = math.sqrt(lo * hi)
        total = np.geomspace(SMALLEST, mid, NUM_TENSORS).round().sum()
        lo, hi = (mid, hi) if total < TOTAL else (lo, mid)
    sizes = np.geomspace(SMALLEST, hi, NUM_TENSORS).round().astype(np.int64)
    np.random.default_rng(SEED).shuffle(sizes)
    return sizes.tolist()


def stats(times):
    return dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), repeats=len(times))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--variant", help="(child of the sweep) the library variant to load; kernel lines only")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()

    import numpy as np
    import torch
    from robust_cvd_amd import api
    if args.variant:
        api.load_library(variant=args.variant)
    from robust_cvd_amd import optimizer, parameter_loss
    from robust_cvd_amd import torch_common as tc
    from robust_cvd_amd.joint_loss import ParameterLoss as TorchParameterLoss
    if not torch.cuda.is_available():
        sys.exit("optimizer_bench: no GPU (nothing here is an estimate)")
    dev = torch.device("cuda", 0)
    lines = []

    def emit(**line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    sizes = tensor_sizes()
    n = sum(sizes)
    emit(kind="parameters", synthetic=True, tensors=len(sizes), elements=n, smallest=min(sizes), largest=max(sizes), dtype="float32",
         spacing="log", seed=SEED, param_chunk=api.PARAM_CHUNK, variant=args.variant, device=torch.cuda.get_device_name(0),
         torch=torch.__version__)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    make = lambda scale=1.0: [torch.randn(s, device=dev, generator=gen) * scale for s in sizes]
    solver = tc.solver(dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def events(fn, calls=1):
        """ms per call: the span between two device events around `calls` back-to-back calls, over `calls`"""
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / calls)
        return stats(out)

    def wall(fn):
        for _ in range(args.warmup):
            fn()
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(1e3 * (time.perf_counter() - t0))
        return stats(out)

    def kernel_line(name, bytes_per_element, fn, kind="kernel"):
        s = events(fn, KERNEL_CALLS)
        gbps = bytes_per_element * n / (s["median_ms"] * 1e-3) / 1e9
        emit(kind=kind, name=name, bytes=bytes_per_element * n, gbps=gbps, hbm_share=gbps * 1e9 / HBM_PEAK, bound="bandwidth",
             param_chunk=api.PARAM_CHUNK, calls_per_window=KERNEL_CALLS, median_ms_is="upper bound on kernel time", **s)

    # ---- kernels: the entry points with prebuilt tables ----
    p, g, m, v = make(), make(1e-2), make(0.0), make(0.0)
    p0 = [t.clone() for t in p]
    for t in p0[::2]:
        t.add_(1e-3)
    grads = [torch.empty_like(t) for t in p]
    one = torch.ones(1, device=dev)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    desc = api.param_desc(0, len(sizes))
    counts = parameter_loss.element_counts(p)
    A = {k: parameter_loss.addresses(x) for k, x in dict(p=p, g=g, m=m, v=v, p0=p0, grads=grads).items()}
    rules = {"adam": api.adam_record(10, 1e-4), "radam": api.radam_record(10, 1e-4), "radam_sgd": api.radam_record(2, 1e-4),
             "moments": api.radam_record(2, 1e-4, degenerated_to_sgd=False)}
    kind = "sweep" if args.variant else "kernel"
    for rule, record in rules.items():
        if args.variant and rule != "adam":
            continue
        assert record.rule == api.PARAM_RULES[rule]
        rec = (api.ParamRecord * len(sizes))(*[record] * len(sizes))
        kernel_line(f"param_step {rule}", 20 if rule == "moments" else 28, lambda: solver._check(solver._fn("param_step_device")(
            solver._h, C.byref(desc), A["p"], A["g"], A["m"], A["v"], counts, rec, stream)), kind)
    kernel_line("parameter_l1 value", 8, lambda: solver._check(solver._fn("parameter_l1_device")(
        solver._h, C.byref(desc), A["p"], A["p0"], counts, C.c_double(LAMBDA), C.c_void_p(total.data_ptr()), None, None, C.c_int32(0),
        stream)), kind)
    kernel_line("parameter_l1 gradient", 12, lambda: solver._check(solver._fn("parameter_l1_device")(
        solver._h, C.byref(desc), A["p"], A["p0"], counts, C.c_double(LAMBDA), None, A["grads"], tc.ptr(one), C.c_int32(0), stream)), kind)
    if args.variant:
        return finish(args, lines)

    # ---- the public surface against what it replaces: wall clock ending in a synchronise, and the device time between events ----
    def with_grads(params):
        for t, gt in zip(params, g):
            t.grad = gt
        return params

    def both(name, fn, replaces=None):
        emit(kind="wall", name=name, replaces=replaces, **wall(fn))
        emit(kind="device", name=name, replaces=replaces, **events(fn))
    params = with_grads([t.clone().requires_grad_(True) for t in p])
    for name in ("Adam", "RAdam"):
        opt = optimizer.create(name, params, lr=1e-4)
        both(f"robust_cvd_amd.optimizer {name}.step()", opt.step)
        del opt
    for label, kw in (("foreach", dict(foreach=True)), ("fused", dict(fused=True))):
        opt = torch.optim.Adam(params, lr=1e-4, **kw)
        both(f"torch.optim.Adam({label}).step()", opt.step, replaces="Adam")
        del opt

    # the reference's RAdam.step restated: per tensor a float copy of the parameter and of the gradient, the moments, the
    # host scalars, the update, the copy back (degenerated_to_sgd, weight_decay 0, the rectified regime from step 6 on)
    state = {}

    def radam_loop(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8):
        with torch.no_grad():
            for t in params:
                grad = t.grad.data.float()
                p32 = t.data.float()
                st = state.get(t)
                if st is None:
                    st = state[t] = dict(step=0, exp_avg=torch.zeros_like(p32), exp_avg_sq=torch.zeros_like(p32))
                exp_avg, exp_avg_sq = st["exp_avg"].type_as(p32), st["exp_avg_sq"].type_as(p32)
                exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
                exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
                st["step"] += 1
                r = api.radam_record(st["step"], lr, (beta1, beta2), eps)
                if r.rule == api.PARAM_RULES["radam"]:
                    p32.addcdiv_(exp_avg, exp_avg_sq.sqrt().add_(eps), value=-r.step)
                else:
                    p32.add_(exp_avg, alpha=-r.step)
                t.data.copy_(p32)
    both("per-tensor RAdam loop (reference semantics, restated)", radam_loop, replaces="RAdam")
    state.clear()
    for t in params:
        t.grad = None

    opt_ns = types.SimpleNamespace(lambda_parameter=LAMBDA)
    for name, criterion in (("robust_cvd_amd.parameter_loss ParameterLoss + backward", parameter_loss.ParameterLoss(p0, opt_ns)),
                            ("torch ParameterLoss (joint_loss.py) + backward", TorchParameterLoss(p0, opt_ns))):
        def call():
            for t in params:
                t.grad = None
            loss, _ = criterion(params)
            loss.backward()
        both(name, call, replaces=None if "robust" in name else "ParameterLoss")

    stopped = None     # the variant whose child failed or ran out of time: nothing is started on the GPU after it
    if not args.no_sweep:
        from robust_cvd_amd import build
        for chunk in SWEEP:
            path = os.path.join(os.path.dirname(build.LIB), f"libcvd_hip_{variant_name(chunk)}.so")
            if stopped is not None:
                emit(kind="sweep", param_chunk=chunk, status=f"not measured: the sweep stopped at chunk {stopped}")
                continue
            if not os.path.exists(path):
                emit(kind="sweep", param_chunk=chunk, status="not measured: the variant library is not built (--build-variants)")
                continue
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", variant_name(chunk), "--warmup",
                                    str(args.warmup), "--repeats", str(args.repeats)], capture_output=True, text=True, timeout=600)
            except subprocess.TimeoutExpired:
                stopped = chunk
                emit(kind="sweep", param_chunk=chunk, status="failed: the child ran out of time")
                continue
            if r.returncode != 0:
                stopped = chunk
                emit(kind="sweep", param_chunk=chunk, status=f"failed: the child ended with status {r.returncode}", stderr=r.stderr[-1000:])
                continue
            for text in r.stdout.splitlines():
                if text.startswith("{") and json.loads(text).get("kind") == "sweep":
                    emit(**json.loads(text))
    finish(args, lines)
    if stopped is not None:
        sys.exit(1)


def finish(args, lines):
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
