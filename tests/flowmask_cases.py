"""Seeded inputs of the flow-mask tests (tests/flowmask_reference.py, test_flowmask_reference.py, test_gpu_flowmask.py and
tests/golden/reference_py/make_flowmask_golden.py): every case is rebuilt from its seeds, the golden file keeps only a digest of
the inputs and the reference's outputs.

A case is (color [F, H, W, C] f32, pairs [U, 2] unordered frame pairs a < b, flow_ab / flow_ba [U, H, W, 2] f32, flow_thresh,
color_thresh).  Flows come from synth.make_dense_flows with 0.35 px of noise and no invalid pixels; colours are smooth sin / cos
fields of position plus a term that drifts with the frame index, so that the photometric check rejects pixels too while the
image gradients (which scale the f32 rounding of the sampling position into the errors) stay small."""
import hashlib

import numpy as np

from robust_cvd_amd import synth

# name: (width, height, video seed, channels, flow_thresh, color_thresh, edge)
CASES = {
    "w96_t1_1": (96, 56, 3, 3, 1.0, 1.0, False),
    "w96_t05_2": (96, 56, 3, 3, 0.5, 2.0, False),
    "w50_t1_1": (50, 31, 4, 3, 1.0, 1.0, False),
    "w96_c1": (96, 56, 3, 1, 1.0, 1.0, False),
    "w50_nan_oob": (50, 31, 4, 3, 1.0, 1.0, True),
}
NUM_FRAMES = 6
ERROR_PAIRS = 4  # unordered pairs per case whose error maps the golden file stores


def colors(num_frames, width, height, channels):
    """[F, H, W, C] f32: a smooth field of position plus a low-frequency term that drifts with the frame index and whose
    amplitude varies over the image, so that every pair keeps some pixels and loses others to the photometric check."""
    x, y = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    out = np.zeros((num_frames, height, width, channels), np.float32)
    for f in range(num_frames):
        for c in range(channels):
            out[f, ..., c] = (0.5 + 0.4 * np.sin(0.2 * x + 0.3 * c) * np.cos(0.17 * y - 0.2 * c)
                              + 0.7 * (1.0 + np.sin(0.11 * x + 0.13 * y)) * np.sin(0.06 * x - 0.05 * y + 0.8 * f + 0.9 * c))
    return out


def unordered_pairs(video):
    """([U, 2] pairs a < b in the order of video.pairs, index of (a, b) and of (b, a) in video.pairs)."""
    directed = [tuple(p) for p in np.asarray(video.pairs).tolist()]
    index = {p: i for i, p in enumerate(directed)}
    un = [p for p in directed if p[0] < p[1]]
    assert all((b, a) in index for a, b in un) and 2 * len(un) == len(directed)
    return (np.array(un, np.int32), np.array([index[p] for p in un]), np.array([index[(b, a)] for a, b in un]))


def make_case(name):
    width, height, seed, channels, ft, ct, edge = CASES[name]
    video = synth.make_video(NUM_FRAMES, width, height, seed=seed)
    flow, _mask = synth.make_dense_flows(video, flow_noise_px=0.35, seed=5, invalid_fraction=0)
    pairs, iab, iba = unordered_pairs(video)
    fab, fba = flow[iab].copy(), flow[iba].copy()
    col = colors(NUM_FRAMES, width, height, channels)
    if edge:  # one pair: NaNs in both flows and in a colour frame, flows that leave the image, targets on the last row / column
        pairs, fab, fba = pairs[:1], fab[:1], fba[:1]
        rng = np.random.default_rng(17)
        fab[0, 3:6, 4:9] = np.nan
        fba[0, 10:12, 20:30, 1] = np.nan
        col = col.copy()
        col[int(pairs[0, 1]), 20:23, 5:8, 1] = np.nan
        fab[0, :, 40:] += rng.uniform(5.0, 60.0, size=(height, width - 40, 1)).astype(np.float32)
        fba[0, :8] -= rng.uniform(5.0, 40.0, size=(8, width, 1)).astype(np.float32)
        gx, gy = np.meshgrid(np.arange(width), np.arange(height))
        fab[0, 24:27, :30, 0] = (width - 1 - gx[24:27, :30]).astype(np.float32)   # x + flow = W - 1 exactly
        fab[0, 27:29, :30, 1] = (height - 1 - gy[27:29, :30]).astype(np.float32)  # y + flow = H - 1 exactly
    return {"color": col, "pairs": pairs, "flow_ab": fab, "flow_ba": fba, "flow_thresh": ft, "color_thresh": ct}


def error_pairs(pairs):
    """Indices of the ERROR_PAIRS unordered pairs whose error maps are stored: the longest baseline first, then the first ones."""
    pairs = np.asarray(pairs)
    longest = int(np.argmax(pairs[:, 1] - pairs[:, 0]))
    rest = [i for i in range(len(pairs)) if i != longest]
    return np.array(sorted([longest] + rest[:ERROR_PAIRS - 1]), np.int64)


def input_digest(case):
    h = hashlib.sha256()
    for k in ("color", "pairs", "flow_ab", "flow_ba"):
        h.update(np.ascontiguousarray(case[k]).tobytes())
    h.update(np.array([case["flow_thresh"], case["color_thresh"]], np.float64).tobytes())
    return h.hexdigest()
