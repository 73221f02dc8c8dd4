"""Seeded inputs of the update-block tests (robust_cvd_amd/csrc/cvd_raftconv.h; tests/test_raftblock_reference.py,
tests/test_gpu_raftblock.py, tests/raftblock_torch_child.py, tests/golden/reference_py/make_raftblock_golden.py).

numpy's generator, not torch's.  Weights and biases U(+-1/sqrt(fan_in)), the default initialisation's range of a Conv2d;
net = tanh(N(0, 1)), inp = relu(N(0, 1)), corr = 4 N(0, 1), flow = 2 N(0, 1); a single convolution's input is drawn like the tensor
its layer reads in the block (relu(N(0, 1)) for an intermediate).  The border pixels of every image are scaled by 3, so that a halo
leaked from a neighbouring row or image shows.  `planted` has zero weights and chosen biases on a few output channels of every
layer, and biases of -100 under the ReLUs on a few others (PLANTED)."""
import hashlib

import numpy as np

COR_PLANES = 324
#             name              out  in   k  (the order of the block's weight and bias lists; the GRU's six: tests/raftgru_cases.py)
LAYERS = (("encoder.convc1", 256, COR_PLANES, 1), ("encoder.convc2", 192, 256, 3), ("encoder.convf1", 128, 2, 7),
          ("encoder.convf2", 64, 128, 3), ("encoder.conv", 126, 256, 3),
          ("gru.convz1", 128, 384, (1, 5)), ("gru.convr1", 128, 384, (1, 5)), ("gru.convq1", 128, 384, (1, 5)),
          ("gru.convz2", 128, 384, (5, 1)), ("gru.convr2", 128, 384, (5, 1)), ("gru.convq2", 128, 384, (5, 1)),
          ("flow_head.conv1", 256, 128, 3), ("flow_head.conv2", 2, 256, 3), ("mask.0", 256, 128, 3), ("mask.2", 576, 256, 1))
PARAMETERS = tuple(l[0] for l in LAYERS)
INDEX = {n: i for i, n in enumerate(PARAMETERS)}
STATE_DICT_KEYS = tuple(f"{n}.{p}" for n in PARAMETERS for p in ("weight", "bias"))

# Single convolutions: name -> (filter, segment channels, out channels per weight, stacked weights, relu, scale, input kind,
#                               (tensor's channels, first channel) of the output or None, (B, H, W))
SENTINEL = np.float32(-12345.0)
_CONV_KINDS = {
    "c1":    (1, (COR_PLANES,), 256, 1, True, 1.0, "corr", None, ((3, 5, 7), (1, 1, 1))),
    "c3seg": (3, (192, 64), 126, 1, True, 1.0, "relu", (128, 0), ((3, 5, 7), (1, 3, 2), (1, 2, 130), (1, 131, 2))),
    "c7":    (7, (2,), 128, 1, True, 1.0, "flow", None, ((1, 1, 1), (1, 3, 2), (2, 9, 11))),
    "c3n2":  (3, (256,), 2, 1, False, 1.0, "relu", None, ((3, 5, 7),)),
    "c3x2":  (3, (128,), 256, 2, True, 1.0, "tanh", None, ((2, 9, 11),)),
    "c1s":   (1, (256,), 576, 1, False, 0.25, "relu", None, ((1, 4, 6),)),
}
CONV_CASES = {f"{kind}_{B}x{H}x{W}": (kind, (B, H, W)) for kind, spec in _CONV_KINDS.items() for B, H, W in spec[-1]}
BLOCK_CASES = {"5x7b3": (3, 5, 7), "9x11": (2, 9, 11), "1x1": (1, 1, 1), "3x2": (1, 3, 2), "2x130": (1, 2, 130), "131x2": (1, 131, 2),
               "planted": (1, 4, 6)}
CONV_MAX_SAMPLES = 32
BLOCK_MAX_SAMPLES = 24
OUTPUTS = ("net", "mask", "delta_flow")

# planted: layer -> ({output channel with ZERO weights: its bias}, output channels with a bias of -100 under the layer's ReLU).
# The output on the first equals relu(bias) exactly (0.25 * bias for mask.2, bias for flow_head.conv2: no ReLU there), on the second 0.
PLANTED = {"encoder.convc1": ({3: 0.75, 70: -0.5, 255: 2.0}, (5, 130)),
           "encoder.convc2": ({0: 1.25, 100: -3.0, 191: 0.5}, (7, 64)),
           "encoder.convf1": ({2: 0.375, 65: -1.0, 127: 4.0}, (9, 33)),
           "encoder.convf2": ({1: 0.625, 63: -0.25}, (8, 40)),
           "encoder.conv": ({4: 1.5, 64: -2.0, 125: 0.125}, (6, 99)),
           "flow_head.conv1": ({10: 0.875, 200: -0.75}, (11, 129)),
           "flow_head.conv2": ({1: -1.625}, ()),
           "mask.0": ({12: 1.125, 255: -4.0}, (13, 77)),
           "mask.2": ({0: 3.0, 64: -1.5, 575: 0.3}, ())}


def _scale_border(a):
    H, W = a.shape[2:]
    border = np.zeros((H, W), bool)
    border[[0, -1], :] = True
    border[:, [0, -1]] = True
    a[:, :, border] *= np.float32(3.0)
    return a


def _draw(rng, kind, shape):
    n = rng.normal(0.0, 1.0, shape)
    a = {"corr": 4.0 * n, "flow": 2.0 * n, "relu": np.maximum(n, 0.0), "tanh": np.tanh(n)}[kind]
    return _scale_border(a.astype(np.float32))


def _conv_parameters(rng, out, cin, k):
    kh, kw = (k, k) if isinstance(k, int) else k
    bound = 1.0 / np.sqrt(float(cin * kh * kw))
    return (rng.uniform(-bound, bound, (out, cin, kh, kw)).astype(np.float32), rng.uniform(-bound, bound, out).astype(np.float32))


def _samples(rng, B, H, W, most):
    M = B * H * W
    if M <= most:
        return np.arange(M, dtype=np.int64)
    fixed = np.unique([0, W - 1, (H - 1) * W, H * W - 1, M - 1])
    rest = np.setdiff1d(np.arange(M), fixed)
    return np.sort(np.r_[fixed, rng.choice(rest, most - len(fixed), replace=False)]).astype(np.int64)


def make_conv_case(name):
    kind, (B, H, W) = CONV_CASES[name]
    k, seg_channels, out, stacked, relu, scale, draw, window, _shapes = _CONV_KINDS[kind]
    rng = np.random.default_rng(sum(name.encode()) + 31700)
    cin = sum(seg_channels)
    params = [_conv_parameters(rng, out, cin, k) for _ in range(stacked)]
    x = _draw(rng, draw, (B, cin, H, W))
    return {"name": name, "x": x, "segments": seg_channels, "weights": [p[0] for p in params], "biases": [p[1] for p in params],
            "k": k, "relu": relu, "scale": scale, "window": window, "samples": _samples(rng, B, H, W, CONV_MAX_SAMPLES)}


def split(case):
    """The case's input as the tuple of its segments (views)."""
    edges = np.cumsum((0,) + tuple(case["segments"]))
    return tuple(case["x"][:, a:b] for a, b in zip(edges[:-1], edges[1:]))


def make_block_case(name):
    B, H, W = BLOCK_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 31701)
    params = [_conv_parameters(rng, out, cin, k) for _n, out, cin, k in LAYERS]
    weights, biases = [p[0] for p in params], [p[1] for p in params]
    net = _draw(rng, "tanh", (B, 128, H, W))
    inp = _draw(rng, "relu", (B, 128, H, W))
    corr = _draw(rng, "corr", (B, COR_PLANES, H, W))
    flow = _draw(rng, "flow", (B, 2, H, W))
    if name == "planted":
        for layer, (zeroed, minus) in PLANTED.items():
            i = INDEX[layer]
            for ch, value in zeroed.items():
                weights[i][ch] = 0.0
                biases[i][ch] = value
            biases[i][list(minus)] = -100.0
    return {"name": name, "net": net, "inp": inp, "corr": corr, "flow": flow, "weights": weights, "biases": biases,
            "samples": _samples(rng, B, H, W, BLOCK_MAX_SAMPLES)}


def input_digest(case):
    hsh = hashlib.sha256()
    arrays = {k: v for k, v in case.items() if isinstance(v, np.ndarray)}
    for i, (w, b) in enumerate(zip(case["weights"], case["biases"])):
        arrays[f"weight{i:02d}"], arrays[f"bias{i:02d}"] = w, b
    for key in sorted(arrays):
        v = arrays[key]
        hsh.update(key.encode())
        hsh.update(str(v.dtype).encode())
        hsh.update(str(v.shape).encode())
        hsh.update(np.ascontiguousarray(v).tobytes())
    return hsh.hexdigest()


def sample_view(case, out):
    """out [B, C, H, W] -> [len(samples), C]: the stored pixels' channels."""
    B, C, H, W = out.shape
    return out.transpose(0, 2, 3, 1).reshape(B * H * W, C)[case["samples"]]
