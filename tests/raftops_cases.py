"""Seeded inputs of the RAFT operator tests (robust_cvd_amd/csrc/cvd_raftops.h; tests/test_raftops_reference.py,
tests/test_gpu_raftops.py, tests/raftops_torch_child.py, tests/golden/reference_py/make_raftops_golden.py).

Correlation cases: feature maps whose entries are multiples of 1/8 in [-2, 2], so that fmap1^T fmap2 is EXACT in f32 in any
summation order (terms are multiples of 1/64 below 4, at most 64 of them): torch's matmul, numpy's and the GPU's give the same
`raw`, and the input digest covers it.  Coordinates are the identity grid plus N(0, 6 px), with planted values in the first cells of
image 0 (PLANTED).  Upsampling cases: a flow of N(0, 3) and logits of N(0, 2), or logits spread over [-100, 100] with both ends hit.
"""
import hashlib

import numpy as np

#         name        B   h   w  dim levels r
CORR = {"square16": (1, 16, 16, 48, 4, 4),    # inexact division by sqrt(48); coarsest level 2 x 2
        "odd17x23": (2, 17, 23, 64, 4, 4),    # pooled sizes 8 x 11, 4 x 5, 2 x 2: dropped rows and columns, batch stride
        "tail16x67": (1, 16, 67, 32, 3, 3)}   # 1072 queries: a ragged last tile of 64; another radius and level count
#         name      N  H  W  logits
UPSAMPLE = {"up5x7": (2, 5, 7, "normal"),
            "up1x1": (1, 1, 1, "normal"),     # every neighbour but the centre is padding
            "up3x4_pm100": (1, 3, 4, "pm100")}
SAMPLED_QUERIES = 256      # queries of odd17x23 / tail16x67 whose reference outputs the fixture stores
ZERO_CELLS = (7, 8, 9, 10, 11, 12)   # planted cells whose windows lie outside every level: exact zeros


def planted(h, w, r, levels):
    """(x, y) of the first 13 cells (row-major) of image 0."""
    far = float((r + 2) << (levels - 1)) + 0.5    # beyond the window at the coarsest level too
    return np.array([
        (3.0, 5.0),                       # 0: exact integers
        (-0.25, 2.5),                     # 1: floor against truncation: the corners are -1 and 0
        (4.5, -3.5),                      # 2: ... -4 and -3
        (-0.999, 4.25),                   # 3..6: one corner just inside each border
        (w - 0.001, 4.25),
        (5.25, -0.999),
        (5.25, h - 0.001),
        (-far, 3.0),                      # 7, 8: windows wholly outside, on every level
        (6.0, h + far + (r << (levels - 1))),
        (1e7, 2.0),                       # 9..12: huge
        (-1e7, 2.0),
        (3.0, 3e9),
        (-3e9, -3e9)], np.float32)


def make_corr_case(name):
    B, h, w, dim, levels, r = CORR[name]
    rng = np.random.default_rng(sum(name.encode()) + 20260)
    fmap1 = (rng.integers(-16, 17, (B, dim, h, w)) / 8.0).astype(np.float32)
    fmap2 = (rng.integers(-16, 17, (B, dim, h, w)) / 8.0).astype(np.float32)
    raw = np.matmul(fmap1.reshape(B, dim, h * w).transpose(0, 2, 1).astype(np.float64), fmap2.reshape(B, dim, h * w).astype(np.float64))
    raw32 = raw.astype(np.float32)
    assert np.array_equal(raw32.astype(np.float64), raw)    # exact in f32
    gy, gx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    coords = np.stack([gx, gy])[None].repeat(B, 0) + rng.normal(0.0, 6.0, (B, 2, h, w)).astype(np.float32)
    coords = np.ascontiguousarray(coords, np.float32)
    pl = planted(h, w, r, levels)
    flat = coords.reshape(B, 2, h * w)
    flat[0, :, :len(pl)] = pl.T
    Q = B * h * w
    # the stored queries: the planted cells, the last query (the ragged tile), and a seeded choice of the rest
    if Q <= SAMPLED_QUERIES:
        queries = np.arange(Q)
    else:
        fixed = np.r_[np.arange(len(pl)), Q - 1]
        rest = np.setdiff1d(np.arange(Q), fixed)
        queries = np.sort(np.r_[fixed, rng.choice(rest, SAMPLED_QUERIES - len(fixed), replace=False)])
    return {"name": name, "B": B, "h": h, "w": w, "dim": dim, "levels": levels, "r": r, "fmap1": fmap1, "fmap2": fmap2,
            "raw": raw32.reshape(Q, h, w), "coords": coords, "queries": queries.astype(np.int64)}


def make_upsample_case(name):
    N, H, W, kind = UPSAMPLE[name]
    rng = np.random.default_rng(sum(name.encode()) + 20261)
    flow = rng.normal(0.0, 3.0, (N, 2, H, W)).astype(np.float32)
    if kind == "normal":
        mask = rng.normal(0.0, 2.0, (N, 576, H, W)).astype(np.float32)
    else:
        mask = rng.uniform(-100.0, 100.0, (N, 576, H, W)).astype(np.float32)
        mask[0, 0::64, 0, 0] = 100.0       # sub-pixel (0, 0) of pixel (0, 0): all nine at the top
        mask[0, 1::64, 0, 0] = -100.0      # ... all nine at the bottom
        mask[0, 2, 0, 0], mask[0, 66, 0, 0] = 100.0, -100.0    # ... the two ends together
    return {"name": name, "flow": flow, "mask": mask}


def input_digest(case):
    hsh = hashlib.sha256()
    for key in sorted(case):
        v = case[key]
        if isinstance(v, np.ndarray):
            hsh.update(key.encode())
            hsh.update(str(v.dtype).encode())
            hsh.update(str(v.shape).encode())
            hsh.update(np.ascontiguousarray(v).tobytes())
    return hsh.hexdigest()


def query_view(case, out):
    """out [B, C, h, w] of the lookup -> [len(queries), C]: the stored queries' channels."""
    B, h, w = case["B"], case["h"], case["w"]
    C = out.shape[1]
    return out.transpose(0, 2, 3, 1).reshape(B * h * w, C)[case["queries"]]
