"""GPU parity of the bilateral depth filter (robust_cvd_amd/csrc/cvd_bilateral.h; DepthVideoProcessor::bilateralFilter,
reference lib/Processor.cpp:183-313) against the numpy restatement tests/bilateral_reference.py, through the Python binding
and through the drop-in module's Op.BilateralFilter.  f32 in the reference's order; the device expf is not glibc's, so the
mean is held to rtol 2e-6 and the median (one of the window's samples) must be exact on >= 99.5 % of the pixels and a
sample of its own window everywhere else."""
import importlib
import os
import shutil
import sys

import numpy as np
import pytest

from robust_cvd_amd import dataset_io, synth
from tests.bilateral_reference import bilateral_filter, bilateral_filter_in_place

pytestmark = pytest.mark.gpu

RTOL = 2e-6
F32 = np.float32


def make_case(n, w, h, seed):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(1.0, 3.0, size=(n, h, w)).astype(F32)
    color = rng.uniform(0.0, 1.0, size=(n, h, w, 3)).astype(F32)
    return depth, color


@pytest.fixture(scope="module")
def solver():
    from robust_cvd_amd.api import Solver
    return Solver(0)


def _window_samples(depth, f, y, x, fr, sr):
    n, h, w = depth.shape
    return depth[max(0, f - fr):min(n, f + fr + 1), max(0, y - sr):min(h, y + sr + 1), max(0, x - sr):min(w, x + sr + 1)]


def check(got, ref, depth, fr, sr, median, first=0):
    assert got.shape == ref.shape and got.dtype == np.float32
    if not median:
        assert np.allclose(got, ref, rtol=RTOL, atol=0), np.abs(got - ref).max()
        return
    same = got == ref
    assert same.mean() >= 0.995, same.mean()
    for f, y, x in zip(*np.nonzero(~same)):
        assert got[f, y, x] in _window_samples(depth, first + f, y, x, fr, sr), (f, y, x)


@pytest.mark.parametrize("n,w,h,fr,sr,ds,cs,median", [
    (7, 64, 40, 2, 0, 0.3, 0.0, False),    # the reference's defaults
    (7, 64, 40, 2, 0, 0.3, 0.0, True),
    (5, 40, 24, 2, 2, 0.3, 0.1, False),    # colour on
    (5, 40, 24, 1, 1, 0.3, 0.5, True),
    (4, 36, 20, 1, 2, 0.0, 0.0, False),    # both sigmas off: box mean / unweighted median
    (4, 36, 20, 1, 1, 0.0, 0.0, True),
    (3, 33, 17, 1, 1, 0.3, 0.0, False),    # rasters that are not tile multiples
    (3, 33, 17, 1, 2, 0.3, 0.2, False),
    (3, 33, 17, 1, 3, 0.3, 0.0, True),
    (4, 20, 12, 2, 3, 0.3, 0.3, False),
    (4, 20, 12, 1, 2, 0.3, 0.3, True),
    (1, 20, 12, 2, 1, 0.3, 0.0, False),    # n = 1
    (1, 20, 12, 2, 1, 0.3, 0.2, True),
])
def test_bilateral_matches_restatement(solver, n, w, h, fr, sr, ds, cs, median):
    depth, color = make_case(n, w, h, seed=n * 13 + sr * 3 + fr)
    got = solver.bilateral_filter(depth, color if cs > 0 else None, fr, sr, ds, cs, median)
    ref = bilateral_filter(depth, color, fr, sr, ds, cs, median)
    check(got, ref, depth, fr, sr, median)


def test_bilateral_output_subrange_is_the_slice_of_the_full_run(solver):
    depth, color = make_case(9, 48, 28, seed=4)
    full = solver.bilateral_filter(depth, color, 2, 1, 0.3, 0.2)
    part = solver.bilateral_filter(depth, color, 2, 1, 0.3, 0.2, first=3, count=4)
    assert part.shape == (4, 28, 48) and np.array_equal(part, full[3:7])
    ref = bilateral_filter(depth, color, 2, 1, 0.3, 0.2, first=3, count=4)
    check(part, ref, depth, 2, 1, False)
    full_m = solver.bilateral_filter(depth, None, 2, 1, 0.3, 0.0, median=True)
    part_m = solver.bilateral_filter(depth, None, 2, 1, 0.3, 0.0, median=True, first=3, count=4)
    assert np.array_equal(part_m, full_m[3:7])


def test_bilateral_median_above_256_samples(solver):
    """r = 4, R = 3: 567 samples per pixel (the wave-per-pixel variant), with and without colour."""
    depth, color = make_case(7, 21, 13, seed=8)
    for cs in (0.0, 0.3):
        got = solver.bilateral_filter(depth, color if cs > 0 else None, 3, 4, 0.3, cs, median=True, first=2, count=3)
        ref = bilateral_filter(depth, color, 3, 4, 0.3, cs, median=True, first=2, count=3)
        check(got, ref, depth, 3, 4, True, first=2)


def test_bilateral_median_rejects_windows_over_the_cap(solver):
    depth, _ = make_case(9, 40, 24, seed=1)
    with pytest.raises(RuntimeError, match="2601 samples"):   # 17^2 x 9
        solver.bilateral_filter(depth, None, 4, 8, median=True)
    # the mean has no cap; the temporal window is clipped to the batch before the count (7^2 x 9 = 441 here)
    solver.bilateral_filter(depth, None, 4, 8)
    solver.bilateral_filter(depth, None, 100, 3, median=True, count=1)


# ---- drop-in: Op.BilateralFilter of lib_python ---------------------------------------------------------------------

F, W, H = 5, 40, 24
SCALES = [1.5, 0.75, 2.0, 1.25, 0.5]


@pytest.fixture(scope="module")
def lib():
    from robust_cvd_amd import build as _b
    d = os.path.dirname(_b.build_lib_python())
    if d not in sys.path:
        sys.path.insert(0, d)
    return importlib.import_module("lib_python")


def _video(lib, tmp_path, colors=True, color_size=(H, W)):
    """Stream 0 with a Global Scale depth transform (scale != 1 per frame) and a second stream "filtered"; colour in
    color_down/ (the "down" stream)."""
    v = synth.make_video(F, W, H, seed=61)
    base = dataset_io.write_dataset(str(tmp_path / "v"), v)
    depth, color = make_case(F, color_size[1], color_size[0], seed=62)
    if colors:
        dataset_io.write_flow_inputs(base, [], [], [], color)
    elif colors is None:   # no "down" stream at all (write_dataset creates an empty color_down/)
        shutil.rmtree(os.path.join(base, "color_down"))
    dv = lib.DepthVideo()
    lib.DepthVideoImporter.importVideo(dv, base, True)
    dv.createDepthStream("depth_midas2", "depth_midas2", [W, H])
    ds = dv.depthStream(0)
    d = lib.XformDescriptor()
    d.depthType = lib.DepthXformType.Global
    d.valueXform = lib.ValueXformType.Scale
    ds.resetDepthXforms(d)
    src, _ = make_case(F, W, H, seed=63)
    for f in range(F):
        ds.frame(f).setDepth(src[f])
        ds.frame(f).depthXform().setParams([SCALES[f]])
    dv.createDepthStream("filtered", "depth_filtered", [W, H])
    return dv, src, color


def _transform(f, x):  # Global Scale: float(double(d) * scale)
    return (np.asarray(x, np.float64) * SCALES[f]).astype(F32)


def _params(lib, frames, depth_stream, sr=1, cs=0.2, median=False):
    p = lib.DepthVideoProcessor.Params()
    p.op = lib.DepthVideoProcessor.Op.BilateralFilter
    p.frameRange.fromString(frames)
    p.depthStream = depth_stream
    p.spatialRadius, p.colorSigma, p.median = sr, cs, median
    p.sourceDepthStream, p.colorStream = 1, 3   # ignored by the reference's filter: source = stream 0, colour = "down"
    return p


def test_drop_in_out_of_place_matches_restatement(lib, tmp_path):
    dv, src, color = _video(lib, tmp_path)
    s0 = dv.depthStream(0)
    depth = np.stack([np.asarray(s0.frame(f).depth()) for f in range(F)])
    assert np.array_equal(depth, np.stack([_transform(f, src[f]) for f in range(F)]))  # (pins the callback below)
    proc = lib.DepthVideoProcessor(dv)
    for median in (False, True):
        proc.process(_params(lib, "1-3", 1, median=median))
        got = np.stack([np.asarray(dv.depthStream(1).frame(f).sourceDepth()) for f in range(1, 4)])
        ref = bilateral_filter(depth, color, 2, 1, 0.3, 0.2, median, first=1, count=3)
        check(got, ref, depth, 2, 1, median, first=1)
    # the source is untouched; bilateralFilter(params) is process(params)
    assert np.array_equal(np.stack([np.asarray(s0.frame(f).sourceDepth()) for f in range(F)]), src)
    before = np.stack([np.asarray(dv.depthStream(1).frame(f).sourceDepth()) for f in range(1, 4)])
    proc.bilateralFilter(_params(lib, "1-3", 1, median=True))
    assert np.array_equal(np.stack([np.asarray(dv.depthStream(1).frame(f).sourceDepth()) for f in range(1, 4)]), before)


def test_drop_in_in_place_is_sequential(lib, tmp_path):
    dv, src, color = _video(lib, tmp_path)
    s0 = dv.depthStream(0)
    depth = np.stack([np.asarray(s0.frame(f).depth()) for f in range(F)])
    proc = lib.DepthVideoProcessor(dv)
    proc.process(_params(lib, "0-3", 0))
    written, after = bilateral_filter_in_place(depth, color, range(4), 2, _transform, 1, 0.3, 0.2)
    got = np.stack([np.asarray(s0.frame(f).sourceDepth()) for f in range(4)])
    ref = np.stack([written[f] for f in range(4)])
    check(got, ref, depth, 2, 1, False)
    assert np.array_equal(np.asarray(s0.frame(4).sourceDepth()), src[4])
    # the sequential result is not the batched one
    batched = bilateral_filter(depth, color, 2, 1, 0.3, 0.2, first=0, count=4)
    assert not np.allclose(got[1:], batched[1:], rtol=1e-4, atol=0)
    assert np.allclose(np.stack([np.asarray(s0.frame(f).depth()) for f in range(4)]), after[:4], rtol=4e-6, atol=0)


def test_drop_in_copy_is_bound(lib, tmp_path):
    dv, src, _ = _video(lib, tmp_path)
    proc = lib.DepthVideoProcessor(dv)
    p = lib.DepthVideoProcessor.Params()
    p.frameRange.fromString("0-4")
    p.sourceDepthStream, p.depthStream = 0, 1
    proc.copy(p)
    a = np.stack([np.asarray(dv.depthStream(1).frame(f).sourceDepth()) for f in range(F)])
    p.op = lib.DepthVideoProcessor.Op.Copy
    dv.depthStream(1).resetDepthXforms(lib.XformDescriptor())
    proc.process(p)
    b = np.stack([np.asarray(dv.depthStream(1).frame(f).sourceDepth()) for f in range(F)])
    assert np.array_equal(a, b) and np.array_equal(a, np.stack([_transform(f, src[f]) for f in range(F)]))


def test_drop_in_rejects_missing_color_and_size_mismatch(lib, tmp_path):
    """A missing "down" stream, a missing colour frame (read even with colorSigma 0), a depth / colour size mismatch."""
    dv, _, _ = _video(lib, tmp_path / "a", colors=None)
    assert not dv.hasColorStream("down")
    with pytest.raises(RuntimeError, match="'down' does not exist"):
        lib.DepthVideoProcessor(dv).process(_params(lib, "0-2", 1))
    dv, _, _ = _video(lib, tmp_path / "b", colors=False)   # the stream's folder without frames
    assert dv.hasColorStream("down")
    with pytest.raises(RuntimeError, match="Could not open"):
        lib.DepthVideoProcessor(dv).process(_params(lib, "0-2", 1, cs=0.0))
    dv, _, _ = _video(lib, tmp_path / "c", color_size=(H, W + 2))
    with pytest.raises(RuntimeError, match="sizes differ"):
        lib.DepthVideoProcessor(dv).process(_params(lib, "0-2", 1, cs=0.0))
