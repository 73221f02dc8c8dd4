"""Seeded inputs of the tests of the backbone's training operators (robust_cvd_amd/csrc/cvd_resnext_grad.h, DESIGN.md §3.22;
tests/test_resnext_grad_reference.py, tests/test_gpu_resnext_grad.py, tests/golden/reference_py/make_resnext_grad_golden.py).  The
smallest shapes at which the kernels can still go wrong: odd sizes, more than one workgroup, every channels-per-group instantiation,
both strides, an unread last row and column at stride 2, 1 x 1 images, several slices of a reduction.  numpy only."""
import hashlib

import numpy as np

from tests import resnext_cases as rc

EPS = rc.EPS
MOMENTUM = 0.1

# ---- batch norm ---------------------------------------------------------------------------------------------------------------------
#  name -> (shape, relu, residual, training, planted constant channel)
NORM_CASES = {
    "plain_2x5x3x7":     ((2, 5, 3, 7), False, False, True, None),
    "relu_1x64x9x11":    ((1, 64, 9, 11), True, False, True, None),
    "residual_2x40x5x7": ((2, 40, 5, 7), False, True, True, None),
    "m2_2x3x1x1":        ((2, 3, 1, 1), False, False, True, None),           # two values per channel
    "constant_channel":  ((2, 5, 3, 7), True, False, True, 1),               # variance exactly zero: invstd = 1 / sqrt(eps)
    "split_2x4x40x60":   ((2, 4, 40, 60), True, False, True, None),          # 4800 values per channel: 5 slices (EXPECTED_NORM_SPLIT)
    "eval_2x5x3x7":      ((2, 5, 3, 7), True, False, False, None),
    "eval_residual":     ((2, 40, 5, 7), False, True, False, None),
}
EXPECTED_NORM_SPLIT = {"plain_2x5x3x7": 1, "relu_1x64x9x11": 1, "split_2x4x40x60": 5}


def make_norm_case(name):
    shape, relu, residual, training, constant = NORM_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 33000)
    N = shape[1]
    c = (rng.normal(0.0, 1.0, shape) * rng.uniform(0.5, 2.0, (1, N, 1, 1)) + rng.normal(0.0, 1.0, (1, N, 1, 1))).astype(np.float32)
    if constant is not None:
        c[:, constant] = np.float32(0.75)
    return {"name": name, "c": c, "norm": rc.norm_vectors(rng, N), "relu": relu, "training": training,
            "residual": rng.normal(0.0, 1.0, shape).astype(np.float32) if residual else None,
            "gy": rng.normal(0.0, 1.0, shape).astype(np.float32)}


# ---- grouped 3 x 3 ------------------------------------------------------------------------------------------------------------------
#  name -> (groups, channels per group, stride, (B, H, W) of the input, forced split of the weight gradient)
GROUPED_CASES = {
    "g4x8_s1_5x7":     (4, 8, 1, (1, 5, 7), 0),
    "g4x16_s1_5x7":    (4, 16, 1, (1, 5, 7), 0),
    "g4x32_s1_5x7":    (4, 32, 1, (1, 5, 7), 0),
    "g4x64_s1_5x7":    (4, 64, 1, (1, 5, 7), 0),
    "g4x8_s2_5x7b2":   (4, 8, 2, (2, 5, 7), 0),
    "g4x16_s2_6x6":    (4, 16, 2, (1, 6, 6), 0),           # the last input row and column are read by no window
    "g4x32_s2_5x7b2":  (4, 32, 2, (2, 5, 7), 0),
    "g4x64_s2_6x6":    (4, 64, 2, (1, 6, 6), 0),
    "g3x8_s1_1x1":     (3, 8, 1, (1, 1, 1), 0),            # G no power of two; the window is all padding but the centre
    "g3x8_s2_1x1":     (3, 8, 2, (1, 1, 1), 0),
    "g4x8_s1_12x13b2_split2": (4, 8, 1, (2, 12, 13), 2),   # 312 output pixels: two chains, a split that really cuts them
    "planted_g4x8_s2_4x5b2":  (4, 8, 2, (2, 4, 5), 0),     # exact
    "planted_g3x16_s1_3x4":   (3, 16, 1, (1, 3, 4), 0),
}


def make_grouped_case(name):
    G, cg, stride, (B, H, W), split = GROUPED_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 33001)
    N, Ho, Wo = G * cg, rc.out_size(H, stride), rc.out_size(W, stride)
    if name.startswith("planted"):
        draw = lambda shape, lo, hi: rng.integers(lo, hi + 1, shape).astype(np.float32)
        return {"name": name, "x": draw((B, N, H, W), -3, 3), "weight": draw((N, cg, 3, 3), -2, 2), "gy": draw((B, N, Ho, Wo), -3, 3),
                "stride": stride, "groups": G, "split": split}
    return {"name": name, "x": rng.normal(0.0, 1.0, (B, N, H, W)).astype(np.float32), "weight": rc.he_weight(rng, (N, cg, 3, 3)),
            "gy": rng.normal(0.0, 1.0, (B, N, Ho, Wo)).astype(np.float32), "stride": stride, "groups": G, "split": split}


# ---- dense convolutions -------------------------------------------------------------------------------------------------------------
#  name -> (in channels, out channels, kernel size, stride, (B, H, W), addend)
DENSE_CASES = {
    "k1_s1_5x7_add":     (5, 7, 1, 1, (2, 5, 7), True),
    "k1_s2_5x7":         (6, 10, 1, 2, (2, 5, 7), False),
    "k1_s2_6x6_add":     (6, 10, 1, 2, (1, 6, 6), True),
    "k1_s2_70_130_9x9":  (70, 130, 1, 2, (2, 9, 9), False),     # more than one 64-channel tile either way
    "stem_9x11":         (3, 64, 7, 2, (1, 9, 11), False),
    "stem_8x8b2":        (3, 64, 7, 2, (2, 8, 8), False),
    "planted_k1_s2_5x6": (4, 6, 1, 2, (2, 5, 6), False),        # exact
    "planted_stem_9x8":  (3, 64, 7, 2, (1, 9, 8), False),
}


def make_dense_case(name):
    Cin, N, k, stride, (B, H, W), add = DENSE_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 33002)
    Ho, Wo = rc.out_size(H, stride), rc.out_size(W, stride)
    if name.startswith("planted"):
        draw = lambda shape, lo, hi: rng.integers(lo, hi + 1, shape).astype(np.float32)
        return {"name": name, "x": draw((B, Cin, H, W), -3, 3), "weight": draw((N, Cin, k, k), -2, 2), "gy": draw((B, N, Ho, Wo), -3, 3),
                "stride": stride, "add": None}
    return {"name": name, "x": rng.normal(0.0, 1.0, (B, Cin, H, W)).astype(np.float32), "weight": rc.he_weight(rng, (N, Cin, k, k)),
            "gy": rng.normal(0.0, 1.0, (B, N, Ho, Wo)).astype(np.float32), "stride": stride,
            "add": rng.normal(0.0, 1.0, (B, Cin, H, W)).astype(np.float32) if add else None}


# ---- max pool -----------------------------------------------------------------------------------------------------------------------
POOL_CASES = dict(rc.POOL_CASES, relu_7x9=(2, 3, 7, 9), all_equal_6x10=(2, 3, 6, 10), four_windows_5x5=(1, 2, 5, 5))


def make_pool_case(name):
    shape = POOL_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 33003)
    x = rng.normal(0.0, 1.0, shape).astype(np.float32)
    if name.startswith("relu"):
        x = np.maximum(x - np.float32(0.2), 0)         # a ReLU output, as the pool's input is: about 58 % exact zeros
        assert (x == 0).mean() >= 0.4
    if name.startswith("all_equal"):
        x[:] = np.float32(0.5)
    if name.startswith("four_windows"):
        x = -np.abs(x)
        x[:, :, 1, 1] = x[:, :, 1, 3] = x[:, :, 3, 3] = np.float32(2.0)      # odd (row, column): the argmax of four windows each
    B, Cn, H, W = shape
    return {"name": name, "x": x, "gy": rng.normal(0.0, 1.0, (B, Cn, rc.out_size(H, 2), rc.out_size(W, 2))).astype(np.float32)}


# ---- one bottleneck ------------------------------------------------------------------------------------------------------------------
#  name -> (form of tests/resnext_cases.py: BLOCK_CASES, training): the three forms in training mode, one in eval mode
BLOCK_CASES = {"layer1_0_train": ("layer1_0", True), "stride2_train": ("stride2", True), "identity_train": ("identity", True),
               "stride2_eval": ("stride2", False)}


def make_block_case(name):
    form, training = BLOCK_CASES[name]
    case = rc.make_block_case(form)
    rng = np.random.default_rng(sum(name.encode()) + 33004)
    B, _, H, W = case["x"].shape
    out = case["params"][2][0].shape[0]
    gy = rng.normal(0.0, 1.0, (B, out, rc.out_size(H, case["stride"]), rc.out_size(W, case["stride"]))).astype(np.float32)
    return {"name": name, "x": case["x"], "weights": [w for w, _ in case["params"]], "norms": [four for _, four in case["params"]],
            "stride": case["stride"], "groups": case["groups"], "training": training, "gy": gy}


# ---- the whole backbone in training mode ---------------------------------------------------------------------------------------------
# SMALL at 2 x 3 x 64 x 64, the loss a random-weighted sum of the four maps.  One seed was tried for this shape; it meets the
# condition delta <= 1e-4 scale for every tensor (tests/resnext_grad_torch_child.py asserts it at run time against stock torch in
# float64, so a draw that misses it fails there and is replaced here).
BACKBONE_SEED = 33010
BACKBONE_SHAPE = (2, 3, 64, 64)


def make_backbone_case():
    blocks, groups, wpg = rc.SMALL
    rng = np.random.default_rng(BACKBONE_SEED)
    params = rc.backbone_parameters(rng, blocks, groups, wpg)
    B, _, H, W = BACKBONE_SHAPE
    images = rng.normal(0.0, 1.0, BACKBONE_SHAPE).astype(np.float32)
    loss = [rng.normal(0.0, 1.0, (B, 256 << k, H >> (k + 2), W >> (k + 2))).astype(np.float32) for k in range(4)]
    return {"blocks": blocks, "groups": groups, "width_per_group": wpg, "images": images, "params": params, "loss_weights": loss}


def input_digest(case):
    hsh = hashlib.sha256()
    for key in sorted(case):
        v = case[key]
        if isinstance(v, np.ndarray):
            hsh.update(key.encode() + str(v.dtype).encode() + str(v.shape).encode() + np.ascontiguousarray(v).tobytes())
        elif isinstance(v, list) and v and isinstance(v[0], np.ndarray):
            for a in v:
                hsh.update(key.encode() + np.ascontiguousarray(a).tobytes())
    return hsh.hexdigest()
