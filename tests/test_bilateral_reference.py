"""Known answers for the numpy restatement of DepthVideoProcessor::bilateralFilter (tests/bilateral_reference.py,
reference lib/Processor.cpp:183-313): the GPU tests compare against it, so it is pinned here on its own (no GPU)."""
import numpy as np

from tests.bilateral_reference import bilateral_filter, bilateral_filter_in_place, filter_frame

F32 = np.float32


def _ramp():
    """3 frames of 4 x 3: depth = 100 k + 10 y + x (exact in f32, as are all the sums below)."""
    k, y, x = np.meshgrid(np.arange(3), np.arange(3), np.arange(4), indexing="ij")
    return (100 * k + 10 * y + x).astype(F32)


def test_constant_input_is_unchanged():
    depth = np.full((4, 5, 7), 2.5, F32)
    color = np.broadcast_to(F32([0.2, 0.4, 0.6]), (4, 5, 7, 3)).copy()
    for median in (False, True):
        for sr, cs in ((0, 0.0), (1, 0.1), (2, 0.5)):
            out = bilateral_filter(depth, color, 2, sr, 0.3, cs, median)
            assert np.array_equal(out, depth), (median, sr, cs)


def test_sigmas_off_give_the_box_mean_with_border_clipping():
    """depthSigma = colorSigma = 0: every weight is 1 (:281), the mean is the box mean of the clipped window."""
    d = _ramp()
    out = bilateral_filter(d, None, 1, 1, depth_sigma=0.0, color_sigma=0.0)
    # frame 0, (x, y) = (0, 0): frames 0-1, rows 0-1, columns 0-1 -> (0 + 1 + 10 + 11) / 4 + 50 = 55.5
    assert out[0, 0, 0] == F32(55.5)
    # frame 1, (3, 2): frames 0-2 (mean 100), rows 1-2 (15), columns 2-3 (2.5)
    assert out[1, 2, 3] == F32(117.5)
    # frame 2, (1, 1): frames 1-2 (150), rows 0-2 (10), columns 0-2 (1)
    assert out[2, 1, 1] == F32(161)
    # interior of the middle frame: the box mean of a linear ramp is its centre value
    assert out[1, 1, 1] == F32(111) and out[1, 1, 2] == F32(112)


def test_sigmas_off_give_the_unweighted_lower_median():
    """Unit weights: half = N / 2 and the first sorted sample with a running count >= N / 2 is the lower median."""
    d = _ramp()
    out = bilateral_filter(d, None, 1, 1, depth_sigma=0.0, color_sigma=0.0, median=True)
    # frame 0, (0, 0): {0, 1, 10, 11, 100, 101, 110, 111}, 4th
    assert out[0, 0, 0] == F32(11)
    # frame 1, (3, 2): {12, 13, 22, 23} + {0, 100, 200}, 12 samples, 6th = 113
    assert out[1, 2, 3] == F32(113)
    # frame 2, (1, 1): 18 samples of frames 1-2, 9th = 122
    assert out[2, 1, 1] == F32(122)


def test_median_breaks_depth_ties_by_weight():
    """std::sort of (depth, weight) pairs (:297): equal depths are ordered by weight, and the running sum follows that order.
    Checked against Python's tuple sort on a case with many exact depth ties, weighted through the colour term."""
    rng = np.random.default_rng(3)
    n, h, w = 3, 6, 7
    depth = rng.integers(1, 4, size=(n, h, w)).astype(F32)       # three distinct depths: ties everywhere
    color = rng.uniform(0, 1, size=(n, h, w, 3)).astype(F32)
    out = filter_frame(depth, color, 1, 1, 1, depth_sigma=0.0, color_sigma=0.4, median=True)
    s2 = F32(0.4) * F32(0.4)
    for y in range(h):
        for x in range(w):
            samples, total = [], F32(0)
            for k in range(n):
                for wy in range(max(0, y - 1), min(h, y + 2)):
                    for wx in range(max(0, x - 1), min(w, x + 2)):
                        e = (color[k, wy, wx] - color[1, y, x]).astype(F32)
                        diff2 = F32(F32(e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
                        ex = F32(F32(0) + F32(-diff2) / s2)
                        wt = F32(np.exp(np.float64(ex))) if ex != 0 else F32(1)
                        samples.append((float(depth[k, wy, wx]), wt))
                        total = F32(total + wt)
            cum, pick = F32(0), None
            for dd, wt in sorted(samples):
                cum = F32(cum + wt)
                if cum >= F32(total / F32(2)):
                    pick = dd
                    break
            assert out[y, x] == F32(pick), (y, x)
    # a hand case: depths (1, 1, 2), colours (0, 1, 0) in the first channel, colorSigma 1.  Pixel 0: pairs (1, 1), (1, e^-1),
    # (2, 1) sort as (1, e^-1), (1, 1), (2, 1); half = 1.18, running 0.37, 1.37 -> depth 1.  Pixel 1: (1, e^-1), (1, 1),
    # (2, e^-1); half = 0.87, running 0.37, 1.37 -> depth 1
    depth = F32([[[1.0, 1.0, 2.0]]])
    color = F32([[[[0, 0, 0], [1, 0, 0], [0, 0, 0]]]])
    got = filter_frame(depth, color, 0, 0, 1, depth_sigma=0.0, color_sigma=1.0, median=True)
    assert got[0, 0] == F32(1) and got[0, 1] == F32(1)


def test_in_place_is_sequential():
    """depthStream = source stream 0: frame 1's window already holds transform(filtered frame 0); frame 0's does not."""
    d = _ramp()
    scale = {0: 2.0, 1: 0.5, 2: 3.0}

    def transform(f, x):
        return (x.astype(np.float64) * scale[f]).astype(F32)

    depth = np.stack([transform(f, d[f]) for f in range(3)])
    written, after = bilateral_filter_in_place(depth, None, [0, 1, 2], 1, transform, 1, depth_sigma=0.0)
    batched = bilateral_filter(depth, None, 1, 1, depth_sigma=0.0)
    assert np.array_equal(written[0], batched[0])
    assert not np.array_equal(written[1], batched[1]) and not np.array_equal(written[2], batched[2])
    # frame 1 = box mean over frames 0 (filtered, re-transformed), 1, 2 (unfiltered)
    step = depth.copy()
    step[0] = transform(0, written[0])
    assert np.array_equal(written[1], filter_frame(step, None, 1, 1, 1, depth_sigma=0.0))
    assert np.array_equal(after[2], transform(2, written[2]))
