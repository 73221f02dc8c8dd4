"""Seeded inputs of the SepConvGRU tests (robust_cvd_amd/csrc/cvd_raftgru.h; tests/test_raftgru_reference.py,
tests/test_gpu_raftgru.py, tests/raftgru_torch_child.py, tests/golden/reference_py/make_raftgru_golden.py).

numpy's generator, not torch's: weights U(+-1/sqrt(1920)) (the default initialisation's range for a fan-in of 384 x 5), biases
U(+-0.02), h = tanh(N(0, 1)), x = relu(N(0, 1)).  The border pixels of every image are scaled by 3 in h and x, so that a halo
leaked from a neighbouring row or image shows.  `trained9x11` scales the weights by 4 and x by 3 (pre-activations to +-16,
saturated gates); `pm100` has the weights of `9x11` and biases of +-100 planted on eight channels of each gate (PLANTED)."""
import hashlib

import numpy as np

HIDDEN, INPUT = 128, 256
PARAMETERS = ("convz1", "convr1", "convq1", "convz2", "convr2", "convq2")     # the order of the weights and biases lists
#        name            B   H    W
CASES = {"5x7b3": (3, 5, 7),            # 105 pixels: one tile of 64 straddles every row and all three images
         "9x11": (2, 9, 11),            # the case behind DESIGN.md §3.16's accumulation-order figures
         "1x1": (1, 1, 1),              # every tap but the centre is padding
         "3x2": (1, 3, 2),              # narrower and shorter than the filter
         "2x130": (1, 2, 130),          # tile edges inside a row
         "131x2": (1, 131, 2),          # ... inside a column
         "trained9x11": (1, 9, 11),
         "pm100": (1, 4, 6)}
MAX_SAMPLES = 64
# pm100: (channels at -100, channels at +100) per gate, the same in both halves.  z = 0 on channels 0..3 in both halves: the output
# is h itself; z = 1 on 4..7 where q is tanh(+-100) = +-1: the output is exactly 1 resp. -1.
PLANTED = {"z": ((0, 1, 2, 3), (4, 5, 6, 7)),
           "r": ((8, 9, 10, 11), (12, 13, 14, 15)),
           "q": ((6, 7, 18, 19), (4, 5, 16, 17))}
PM100_KEEPS_H = (0, 1, 2, 3)
PM100_PLUS_ONE = (4, 5)
PM100_MINUS_ONE = (6, 7)


def weight_shape(name):
    return (HIDDEN, HIDDEN + INPUT) + ((1, 5) if name.endswith("1") else (5, 1))


def _parameters(name):
    rng = np.random.default_rng(sum(name.encode()) + 20270)
    bound = 1.0 / np.sqrt(5.0 * (HIDDEN + INPUT))
    weights = [rng.uniform(-bound, bound, weight_shape(n)).astype(np.float32) for n in PARAMETERS]
    biases = [rng.uniform(-0.02, 0.02, HIDDEN).astype(np.float32) for _ in PARAMETERS]
    return weights, biases


def make_case(name):
    B, H, W = CASES[name]
    weights, biases = _parameters("9x11" if name == "pm100" else name)
    rng = np.random.default_rng(sum(name.encode()) + 20271)
    h = np.tanh(rng.normal(0.0, 1.0, (B, HIDDEN, H, W))).astype(np.float32)
    x = np.maximum(rng.normal(0.0, 1.0, (B, INPUT, H, W)), 0.0).astype(np.float32)
    border = np.zeros((H, W), bool)
    border[[0, -1], :] = True
    border[:, [0, -1]] = True
    h[:, :, border] *= np.float32(3.0)
    x[:, :, border] *= np.float32(3.0)
    if name == "trained9x11":
        weights = [w * np.float32(4.0) for w in weights]
        x *= np.float32(3.0)
    if name == "pm100":
        for i, n in enumerate(PARAMETERS):
            minus, plus = PLANTED[n[4]]
            biases[i][list(minus)] = -100.0
            biases[i][list(plus)] = 100.0
    M = B * H * W
    if M <= MAX_SAMPLES:
        samples = np.arange(M)
    else:
        fixed = np.unique([0, W - 1, (H - 1) * W, H * W - 1, M - 1])
        rest = np.setdiff1d(np.arange(M), fixed)
        samples = np.sort(np.r_[fixed, rng.choice(rest, MAX_SAMPLES - len(fixed), replace=False)])
    return {"name": name, "h": h, "x": x, "weights": weights, "biases": biases, "samples": samples.astype(np.int64)}


def input_digest(case):
    hsh = hashlib.sha256()
    arrays = {"h": case["h"], "x": case["x"], "samples": case["samples"]}
    for n, w, b in zip(PARAMETERS, case["weights"], case["biases"]):
        arrays[n + ".weight"], arrays[n + ".bias"] = w, b
    for key in sorted(arrays):
        v = arrays[key]
        hsh.update(key.encode())
        hsh.update(str(v.dtype).encode())
        hsh.update(str(v.shape).encode())
        hsh.update(np.ascontiguousarray(v).tobytes())
    return hsh.hexdigest()


def sample_view(case, out):
    """out [B, 128, H, W] -> [len(samples), 128]: the stored pixels' channels."""
    B, C, H, W = out.shape
    return out.transpose(0, 2, 3, 1).reshape(B * H * W, C)[case["samples"]]
