"""Seeded inputs of the consistency-loss tests (robust_cvd_amd/csrc/cvd_consistency.h) and the list of
(case, distance, lambdas) combinations the fixture tests/golden/reference_py/consistency_golden.npz records.

Every real input is a float32-representable number held in float64, so the f32 and the f64 kernels (and the reference's f32 and
f64 runs) see the same inputs.  The warp is generated in the reference's normalised units as multiples of 2^-12: times W/2 or
H/2 (what the reference does in place on every call) is then exact in both precisions, and `warp` below, the pixel offsets the
kernels take, is exactly what the reference adds to its pixel grid.

The frames carry different depth scales (a non-converged state): the disparity and depth-ratio errors stay away from their sign
kinks; `check_kinks` (tests/consistency_reference.py) asserts the distance for every weighted sample.
"""
import hashlib

import numpy as np

# name -> shape, frames, pairs, warp, flow noise (px), seed
CASES = {
    # 851 pixels: a ragged last block and the one-pixel path; frame 0 and 1 are ref and target of several pairs
    "odd": dict(H=23, W=37, F=4, pairs=[(0, 1), (1, 2), (0, 3)], warp=True, sigma=3.0, seed=9101, masked=(1, 1)),
    # the four-pixel path, no warp
    "portrait": dict(H=40, W=24, F=4, pairs=[(0, 1), (3, 2)], warp=False, sigma=2.0, seed=9122, masked=None),
    # the reference's own layout: F = 2 B, pairs (2 b, 2 b + 1)
    "batch": dict(H=24, W=40, F=6, pairs=[(0, 1), (2, 3), (4, 5)], warp=True, sigma=2.0, seed=9113, masked=None),
}

DEFAULT_LAMBDAS = (1.0, 0.0, 100.0)
# (case, distance, scale, alpha, lambdas)
COMBOS = (
    [("odd", d, 1.0, 1.0, DEFAULT_LAMBDAS) for d in ("l1", "l2", "smooth_l1", "cauchy")]
    + [("odd", "general", 0.7, -1.5, DEFAULT_LAMBDAS)]
    + [("odd", "l1", 1.0, 1.0, lam) for lam in ((1.0, 0.5, 0.0), (0.0, 0.0, 100.0), (1.0, 0.5, 100.0))]
    + [(c, "l1", 1.0, 1.0, DEFAULT_LAMBDAS) for c in ("portrait", "batch")]
    + [(c, "cauchy", 1.0, 1.0, (1.0, 0.5, 100.0)) for c in ("portrait", "batch")]
)


def combo_key(combo):
    case, dist, scale, alpha, lam = combo
    name = f"{case}-{dist}-{lam[0]:g}_{lam[1]:g}_{lam[2]:g}"
    return name + (f"-a{alpha:g}-s{scale:g}" if dist == "general" else "")


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _rotation(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


_CACHE = {}


def make_case(name):
    """dict of float64 arrays: depth [F, H, W], extrinsics [F, 3, 4], intrinsics [F, 4], warp [F, 2, H, W] pixel offsets or None,
    warp_norm (the reference's metadata["warp"], normalised) or None, pairs [P, 2] int32, flow_ab / flow_ba [P, 2, H, W],
    weight_ab / weight_ba [P, H, W].  Cached: callers must not modify it."""
    if name in _CACHE:
        return _CACHE[name]
    c = CASES[name]
    H, W, F = c["H"], c["W"], c["F"]
    pairs = np.array(c["pairs"], np.int32)
    P = len(pairs)
    rng = np.random.default_rng(c["seed"])
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = np.zeros((F, H, W))
    ext = np.zeros((F, 3, 4))
    intr = np.zeros((F, 4))
    for f in range(F):
        ph = rng.uniform(0, 2 * np.pi, 2)
        depth[f] = (1.0, 1.4)[f % 2] * (1.0 + 0.1 * (f // 2)) * (3.0 + 0.5 * np.sin(xx / W * 4.0 + ph[0]) + 0.4 * np.cos(yy / H * 3.0 + ph[1])
                                       + rng.normal(0.0, 0.05, (H, W)))
        ext[f, :, :3] = _rotation(rng.normal(0.0, np.deg2rad(2.0), 3))
        ext[f, :, 3] = rng.normal(0.0, 0.08, 3)
        intr[f] = (0.9 * W * (1 + rng.uniform(-0.05, 0.05)), 0.9 * W * (1 + rng.uniform(-0.05, 0.05)),
                   W / 2.0 + rng.uniform(-0.5, 0.5), H / 2.0 + rng.uniform(-0.5, 0.5))
    warp_norm = warp = None
    if c["warp"]:
        warp_norm = np.round(rng.normal(0.0, 0.02, (F, 2, H, W)) * 4096.0) / 4096.0
        warp = warp_norm * np.array([W / 2.0, H / 2.0]).reshape(1, 2, 1, 1)   # exact in f32 and in f64
        assert np.array_equal(warp, _f32(warp)) and np.array_equal(warp_norm, _f32(warp_norm))
    flows = [rng.normal(0.0, c["sigma"], (P, 2, H, W)) for _ in range(2)]
    weights = []
    for _ in range(2):
        u = rng.uniform(0, 1, (P, H, W))
        w = np.where(u < 0.8, 1.0, np.where(u < 0.9, 0.0, rng.uniform(0.05, 1.0, (P, H, W))))   # 80 % ones, 10 % zeros, 10 % reals
        weights.append(w)
    if c["masked"] is not None:
        p, k = c["masked"]
        weights[k][p] = 0.0    # one direction of one pair fully masked
    case = dict(name=name, H=H, W=W, F=F, P=P, pairs=pairs, depth=_f32(depth), extrinsics=_f32(ext), intrinsics=_f32(intr),
                warp=warp, warp_norm=warp_norm, flow_ab=_f32(flows[0]), flow_ba=_f32(flows[1]), weight_ab=_f32(weights[0]),
                weight_ba=_f32(weights[1]))
    if name == "odd":
        # matches leave the image on all four sides, with weight
        sides = np.zeros(4, bool)
        for p in range(P):
            for k, (fl, wt) in enumerate(((case["flow_ab"], case["weight_ab"]), (case["flow_ba"], case["weight_ba"]))):
                r = pairs[p][k]
                mx = xx + warp[r, 0] + fl[p, 0]
                my = yy + warp[r, 1] + fl[p, 1]
                u, v = mx * W / (W - 1) - 0.5, my * H / (H - 1) - 0.5
                on = wt[p] > 0
                sides |= np.array([(on & (u < 0)).any(), (on & (u > W - 1)).any(), (on & (v < 0)).any(), (on & (v > H - 1)).any()])
        assert sides.all(), sides
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _CACHE[name] = case
    return case


def case_args(case, dtype=np.float64):
    """Positional arguments of Solver.consistency_loss / the restatement for a case, in `dtype`."""
    t = lambda a: None if a is None else np.ascontiguousarray(a, dtype=dtype)
    return (t(case["depth"]), t(case["extrinsics"]), t(case["intrinsics"]), case["pairs"], t(case["flow_ab"]), t(case["flow_ba"]),
            t(case["weight_ab"]), t(case["weight_ba"]), t(case["warp"]))


def digest(case):
    """sha256 over the inputs (float64 bytes, fixed order): the fixture records it, the tests compare."""
    h = hashlib.sha256()
    for k in ("depth", "extrinsics", "intrinsics", "warp", "pairs", "flow_ab", "flow_ba", "weight_ab", "weight_ba"):
        a = case[k]
        h.update(k.encode())
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()
