#!/usr/bin/env python3
"""Measure the fine-tuning batches served from the device-resident dataset (robust_cvd_amd/csrc/cvd_batch.h) on
the GPU.

    python tools/dataset_bench.py --out profiles/dataset_bench.json

Every output line is one measurement; nothing here is a pass / fail bar.  Without a GPU the tool fails: nothing is an estimate.
  * kernel: a 300-frame store of 384 x 224 frames filled from a seed (no files), one batch of (B, N) in (2, 2), (2, 6), (16, 6)
    with scale maps and warps: `kernel_ms` is the HIP-event time around one call of the device entry point (device indices in,
    device tensors out; the launch overhead is inside, so it is an upper bound on the kernel's own time), the median of --batches batches (at least 200) after --warmup; `bytes` is what the batch moves, computed here from the shapes (every
    output written once, every copied element read once in its stored width: a mask byte per mask float, nothing for the
    dummies); `hbm_share` = bytes / time over the 8 TB/s peak, `copy_share` over the 6.29 TB/s a plain float4 copy reaches.
  * wall: host clock per batch of `VideoDataset.loader` against a file-reading baseline in the same run, alternating epochs: a
    torch.utils.data.DataLoader (4 workers, pin_memory) over this package's own readers (robust_cvd_amd.video_dataset.load_color /
    load_flow / load_mask: the work the reference's dataset does per sample) followed by .to(device), on a 60-frame dataset
    written to a temporary directory.  The workers read files and never touch the GPU.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK, COPY_RATE = 8.0e12, 6.29e12
H, W, STORE_FRAMES, FILE_FRAMES = 224, 384, 300, 60
SHAPES = ((2, 2), (2, 6), (16, 6))


def batch_bytes(B, N, npx, dummies=0):
    """Bytes one batch moves with scale maps and warps; `dummies`: neighbour pairs of boundary frames in it (written, not read)."""
    real_neighbors = B * (N - 2) - 2 * dummies
    color = (2 * B + real_neighbors) * 3 * npx * 4
    flows = (2 * B + real_neighbors) * 2 * npx * 4
    masks_read = (2 * B + real_neighbors) * npx
    tables = B * N * 3 * npx * 4                      # one scale plane and two warp planes per frame
    read = color + flows + masks_read + tables
    written = B * N * 3 * npx * 4 + B * N * 2 * npx * 4 + B * N * npx * 4 + tables
    small = B * N * 16 * 4 * 2 + B * 6 * 8 + B * 2 * 4
    return read + written + small


def stats(times):
    return dict(median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times), repeats=len(times))


def kernel_lines(args, emit):
    import ctypes as C

    import numpy as np
    import torch
    from robust_cvd_amd import api
    from robust_cvd_amd import torch_common as tc
    dev = torch.device("cuda", 0)
    s = tc.solver(dev)
    rng = np.random.default_rng(1)
    F, npx = STORE_FRAMES, H * W
    for N in (2, 6):
        pairs = [(k, k + 1) for k in range(F - 1)]
        directed = [p for a, b in pairs for p in ((a, b), (b, a))]
        s.dataset_create(F, H, W, directed, pairs, N == 6)
        for f0 in range(0, F, 50):
            s.dataset_set_colors(f0, rng.random((50, H, W, 3), np.float32))
        for q0 in range(0, len(directed), 46):
            n = min(46, len(directed) - q0)
            s.dataset_set_flows(q0, rng.standard_normal((n, H, W, 2)).astype(np.float32), rng.integers(0, 2, (n, H, W)).astype(np.uint8) * 255)
        s.dataset_set_cameras(rng.random((F, 3, 4), np.float32), rng.random((F, 4), np.float32))
        s.dataset_set_maps(rng.random((F, H, W), np.float32), rng.random((F, 2, H, W), np.float32))
        for B, n in SHAPES:
            if n != N:
                continue
            # device indices in, device tensors out: the device entry point between two events on torch's stream
            shapes = api.dataset_batch_shapes(B, N, H, W, 2, True)
            flat = {k: torch.empty(shape, dtype=getattr(torch, dtype), device=dev) for k, (shape, dtype) in shapes.items()}
            out = api.dataset_batch_out({k: t.data_ptr() for k, t in flat.items()})
            stream = torch.cuda.current_stream().cuda_stream
            order = torch.Generator(device=dev)
            order.manual_seed(2)
            times = []
            for k in range(args.warmup + args.batches):
                idx = torch.randint(1, len(pairs) - 1, (B,), device=dev, generator=order)      # interior samples: no dummies
                begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                begin.record()
                s._check(s._fn("dataset_batch_device")(s._h, C.c_int32(B), C.c_void_p(idx.data_ptr()), C.byref(out), C.c_void_p(stream)))
                end.record()
                end.synchronize()
                if k >= args.warmup:
                    times.append(begin.elapsed_time(end))
            assert s.dataset_bad_indices() == 0
            st = stats(times)
            nbytes = batch_bytes(B, N, npx)
            rate = nbytes / (st["median_ms"] * 1e-3)
            emit(dict(kind="kernel", B=B, N=N, height=H, width=W, store_frames=F, bytes=nbytes, kernel_ms=st, gbps=rate / 1e9,
                      hbm_share=rate / HBM_PEAK, copy_share=rate / COPY_RATE))
    s.dataset_clear()


class FileDataset:
    """What the reference's VideoDataset does per sample (N = 2), with this package's readers; CPU tensors."""

    def __init__(self, plan):
        self.plan = plan

    def __len__(self):
        return len(self.plan["pairs"])

    def __getitem__(self, i):
        import numpy as np
        import torch
        from robust_cvd_amd import video_dataset as vd
        a, b = self.plan["pairs"][i]
        p = self.plan
        chw = lambda x: torch.from_numpy(np.ascontiguousarray(np.transpose(x, (2, 0, 1))))
        images = torch.stack([chw(vd.load_color(p["color_fmt"].format(k))) for k in (a, b)])
        flows = [chw(vd.load_flow(p["flow_fmt"].format(s, t))) for s, t in ((a, b), (b, a))]
        masks = [torch.from_numpy((vd.load_mask(p["mask_fmt"].format(s, t)) > 0).astype(np.float32))[None] for s, t in ((a, b), (b, a))]
        return images, {"geometry_consistency": {"indices": torch.tensor([a, b]), "flows": flows, "masks": masks}}


def to_device(x, dev):
    if isinstance(x, dict):
        return {k: to_device(v, dev) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [to_device(v, dev) for v in x]
    return x.to(dev, non_blocking=True)


def wall_lines(args, emit):
    import numpy as np
    import torch
    from robust_cvd_amd import dataset_io
    from robust_cvd_amd import video_dataset as vd
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    F = FILE_FRAMES
    pairs = [(k, k + 1) for k in range(F - 1)]
    directed = [p for a, b in pairs for p in ((a, b), (b, a))]
    with tempfile.TemporaryDirectory() as tmp:
        dataset_io.write_flow_inputs(tmp, directed, [rng.standard_normal((H, W, 2)).astype(np.float32) for _ in directed],
                                     [rng.integers(0, 2, (H, W)).astype(np.uint8) * 255 for _ in directed],
                                     rng.random((F, H, W, 3), np.float32))
        meta = os.path.join(tmp, "metadata.npz")
        np.savez(meta, extrinsics=rng.random((F, 3, 4), np.float32), intrinsics=rng.random((F, 4), np.float32))
        t0 = time.perf_counter()
        ours = vd.VideoDataset(tmp, list(range(F)), None, False, meta, "colmap", device=dev)
        torch.cuda.synchronize()
        emit(dict(kind="load", frames=F, pairs=len(directed), seconds=time.perf_counter() - t0))
        baseline = torch.utils.data.DataLoader(FileDataset(vd.plan(tmp, list(range(F)), None, False)), batch_size=args.batch_size,
                                               shuffle=True, num_workers=4, pin_memory=True)
        per = {"loader": [], "baseline": []}
        for _epoch in range(args.epochs):
            for name, it in (("loader", lambda: ours.loader(args.batch_size, shuffle=True)),
                             ("baseline", lambda: (to_device(b, dev) for b in baseline))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 0
                for _images, _meta in it():
                    n += 1
                torch.cuda.synchronize()
                per[name].append((time.perf_counter() - t0) * 1e3 / n)
        for name, times in per.items():
            emit(dict(kind="wall", what=name, batch_size=args.batch_size, frames=F, ms_per_batch=stats(times)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_bench.json"))
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--skip-wall", action="store_true")
    args = ap.parse_args()
    args.batches = max(args.batches, 200)
    import torch  # noqa: F401  (first: the process then holds one HIP runtime, torch's)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
    kernel_lines(args, emit)
    if not args.skip_wall:
        wall_lines(args, emit)
    with open(args.out, "w") as f:
        json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
