"""Seeded inputs of the encoder tests (robust_cvd_amd/csrc/cvd_raftenc.h; tests/test_raftenc_reference.py,
tests/test_gpu_raftenc.py, tests/raftenc_torch_child.py, tests/golden/reference_py/make_raftenc_golden.py).

numpy's generator, not torch's.  Weights and biases U(+-1/sqrt(fan_in)); batch-norm vectors running_mean ~ N(0, 0.5), running_var ~
U(0.5, 2), weight ~ U(0.5, 1.5), bias ~ N(0, 0.3); images U(-1, 1), intermediates relu(N(0, 1)); the border pixels of every image are
scaled by 3, so that a halo leaked from a neighbouring row or image shows.  The planted cases have zero weights and chosen biases on
a few output channels and biases of -100 under the ReLU on others (PLANTED)."""
import hashlib

import numpy as np

from tests import raftblock_cases as bc

#           name                       out   in  k  stride   (the order of the encoder's weight and bias lists; conv2: out = output_dim)
LAYERS = (("conv1", 64, 3, 7, 2),
          ("layer1.0.conv1", 64, 64, 3, 1), ("layer1.0.conv2", 64, 64, 3, 1), ("layer1.1.conv1", 64, 64, 3, 1), ("layer1.1.conv2", 64, 64, 3, 1),
          ("layer2.0.conv1", 96, 64, 3, 2), ("layer2.0.conv2", 96, 96, 3, 1), ("layer2.0.downsample.0", 96, 64, 1, 2),
          ("layer2.1.conv1", 96, 96, 3, 1), ("layer2.1.conv2", 96, 96, 3, 1),
          ("layer3.0.conv1", 128, 96, 3, 2), ("layer3.0.conv2", 128, 128, 3, 1), ("layer3.0.downsample.0", 128, 96, 1, 2),
          ("layer3.1.conv1", 128, 128, 3, 1), ("layer3.1.conv2", 128, 128, 3, 1),
          ("conv2", 256, 128, 1, 1))
PARAMETERS = tuple(l[0] for l in LAYERS)
# norm i stands behind convolution i; layerX.0.norm3 is registered a second time as layerX.0.downsample.1
NORMS = ("norm1", "layer1.0.norm1", "layer1.0.norm2", "layer1.1.norm1", "layer1.1.norm2", "layer2.0.norm1", "layer2.0.norm2",
         "layer2.0.norm3", "layer2.1.norm1", "layer2.1.norm2", "layer3.0.norm1", "layer3.0.norm2", "layer3.0.norm3", "layer3.1.norm1",
         "layer3.1.norm2")
NORM_VECTORS = ("weight", "bias", "running_mean", "running_var")
EPS = 1e-5
OUTPUT_DIM = 256


def encoder_keys(prefix, norm):
    """The state-dict keys of the reference's BasicEncoder in its order: the module's norm1 first, then conv1, the blocks (conv1,
    conv2, norm1, norm2, norm3, downsample.0, downsample.1) and conv2; an instance norm has no entries."""
    def norm_keys(name):
        return [f"{prefix}{name}.{v}" for v in NORM_VECTORS + ("num_batches_tracked",)] if norm == "batch" else []

    def conv_keys(name):
        return [f"{prefix}{name}.weight", f"{prefix}{name}.bias"]
    keys = norm_keys("norm1") + conv_keys("conv1")
    for layer in (1, 2, 3):
        for blk in (0, 1):
            b = f"layer{layer}.{blk}."
            keys += conv_keys(b + "conv1") + conv_keys(b + "conv2") + norm_keys(b + "norm1") + norm_keys(b + "norm2")
            if blk == 0 and layer > 1:
                keys += norm_keys(b + "norm3") + conv_keys(b + "downsample.0") + norm_keys(b + "downsample.1")
    return keys + conv_keys("conv2")


RAFT_STATE_DICT_KEYS = tuple(encoder_keys("fnet.", "instance") + encoder_keys("cnet.", "batch")
                             + ["update_block." + k for k in bc.STATE_DICT_KEYS])

# Single convolutions: kind -> (filter, stride, in channels, out channels, epilogue form, input kind)
# forms: plain | relu_res (no norm) | bn (the downsample branch) | bn_relu | bn_relu_res
CONV_KINDS = {
    "c7s2":     (7, 2, 3, 64, "bn_relu", "image"),
    "c3_64":    (3, 1, 64, 64, "bn_relu_res", "relu"),
    "c3s2_96":  (3, 2, 64, 96, "plain", "relu"),
    "c3s2_128": (3, 2, 96, 128, "bn_relu", "relu"),
    "c1s2_96":  (1, 2, 64, 96, "bn", "relu"),
    "c1s2_128": (1, 2, 96, 128, "bn", "relu"),
    "c3_96":    (3, 1, 96, 96, "relu_res", "relu"),
    "c3_128":   (3, 1, 128, 128, "bn_relu_res", "relu"),
    "c1_256":   (1, 1, 128, 256, "plain", "relu"),
}
# 3 x 5 x 7: 105 output pixels at stride 1 and 36 at stride 2, no multiple of the tile of 64, over three images; 5 x 7 and 6 x 8:
# the last tap row and column of a strided filter fall in the padding in one and not in the other
CONV_SHAPES = ((1, 1, 1), (1, 2, 3), (3, 5, 7), (2, 6, 8), (1, 2, 130), (1, 131, 2))
CONV_CASES = {f"{kind}_{B}x{H}x{W}": (kind, (B, H, W)) for kind in CONV_KINDS for B, H, W in CONV_SHAPES}
CONV_CASES["planted_3x5x7"] = ("planted", (3, 5, 7))
# planted: a 3 x 3, 64 -> 64 convolution with ReLU and no norm: {output channel with ZERO weights: its bias}, channels with bias -100
PLANTED = ({0: 0.75, 31: -0.5, 63: 2.0}, (5, 40))
CONV_KINDS["planted"] = (3, 1, 64, 64, "relu", "relu")

# Instance norm: name -> (shape, relu, residual, input kind)
NORM_CASES = {
    "in_2":      ((2, 3, 1, 2), False, False, "normal"),
    "in_35":     ((2, 3, 5, 7), True, True, "normal"),
    "in_35p":    ((1, 2, 5, 7), True, False, "normal"),
    "in_9100":   ((1, 2, 130, 70), True, False, "normal"),
    "in_const":  ((1, 2, 5, 7), False, False, "constant"),
    "in_offset": ((1, 2, 13, 9), False, True, "offset"),
}

# Whole encoders: name -> (image shape, norm mode)
ENCODER_SHAPES = {"9x9": (1, 3, 9, 9), "13x9b2": (2, 3, 13, 9), "16x24b3": (3, 3, 16, 24), "40x56": (1, 3, 40, 56)}
ENCODER_CASES = {f"{norm}_{name}": (shape, norm) for name, shape in ENCODER_SHAPES.items() for norm in ("none", "instance", "batch")}
ENCODER_CASES["planted"] = ((1, 3, 16, 24), "none")
PLANTED_ENCODER = {5: 0.75, 200: -1.5}      # conv2 (no ReLU behind it): output channel with zero weights -> its bias

# Whole RAFT (torch child): name -> (image shape, iters)
RAFT_CASES = {"128x128": ((1, 3, 128, 128), 2), "136x160b2": ((2, 3, 136, 160), 3)}
MAX_SAMPLES = 16


def _scale_border(a):
    return bc._scale_border(a)


def _draw(rng, kind, shape):
    if kind == "image":
        a = rng.uniform(-1.0, 1.0, shape)
    elif kind == "relu":
        a = np.maximum(rng.normal(0.0, 1.0, shape), 0.0)
    else:
        a = rng.normal(0.0, 1.0, shape)
    return _scale_border(a.astype(np.float32))


def _conv_parameters(rng, out, cin, k):
    return bc._conv_parameters(rng, out, cin, k)


def _norm_vectors(rng, n):
    """(weight, bias, running_mean, running_var) of a batch norm over n channels."""
    mean = rng.normal(0.0, 0.5, n).astype(np.float32)
    var = rng.uniform(0.5, 2.0, n).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, n).astype(np.float32)
    beta = rng.normal(0.0, 0.3, n).astype(np.float32)
    return [gamma, beta, mean, var]


def out_size(n, stride):
    return (n - 1) // stride + 1


def make_conv_case(name):
    kind, (B, H, W) = CONV_CASES[name]
    k, stride, cin, cout, form, draw = CONV_KINDS[kind]
    rng = np.random.default_rng(sum(name.encode()) + 31800)
    weight, bias = _conv_parameters(rng, cout, cin, k)
    x = _draw(rng, draw, (B, cin, H, W))
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    norm = _norm_vectors(rng, cout) if form.startswith("bn") else None
    residual = _draw(rng, "relu", (B, cout, Ho, Wo)) if form.endswith("res") else None
    if kind == "planted":
        zeroed, minus = PLANTED
        for ch, value in zeroed.items():
            weight[ch] = 0.0
            bias[ch] = value
        bias[list(minus)] = -100.0
    return {"name": name, "x": x, "weight": weight, "bias": bias, "k": k, "stride": stride, "norm": norm,
            "relu": "relu" in form, "residual": residual, "samples": bc._samples(rng, B, Ho, Wo, MAX_SAMPLES)}


def make_norm_case(name):
    shape, relu, with_residual, kind = NORM_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 31801)
    x = rng.normal(0.0, 1.0, shape)
    if kind == "constant":
        x[:, 0] = 3.5
    elif kind == "offset":
        x += 1000.0
    x = x.astype(np.float32)
    residual = _draw(rng, "relu", shape) if with_residual else None
    B, _, H, W = shape
    return {"name": name, "x": x, "relu": relu, "residual": residual, "samples": bc._samples(rng, B, H, W, MAX_SAMPLES)}


def encoder_parameters(rng, output_dim=OUTPUT_DIM):
    """(weights[16], biases[16], norms[15][4]) in the entry point's order."""
    weights, biases = [], []
    for name, out, cin, k, _stride in LAYERS:
        w, b = _conv_parameters(rng, output_dim if name == "conv2" else out, cin, k)
        weights.append(w)
        biases.append(b)
    norms = [_norm_vectors(rng, LAYERS[i][1]) for i in range(15)]
    return weights, biases, norms


def make_encoder_case(name):
    shape, norm = ENCODER_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 31802)
    weights, biases, norms = encoder_parameters(rng)
    images = _draw(rng, "image", shape)
    if name == "planted":
        for ch, value in PLANTED_ENCODER.items():
            weights[15][ch] = 0.0
            biases[15][ch] = value
    B, _, H, W = shape
    return {"name": name, "images": images, "norm_mode": norm, "weights": weights, "biases": biases, "norms": norms,
            "samples": bc._samples(rng, B, out_size(H, 8), out_size(W, 8), MAX_SAMPLES)}


def make_raft_case(name):
    """Two images in 0..255 (blocks of 8 x 8 with noise; the second the first moved by two pixels, with its own noise) and the whole
    network's parameters under the reference's 179 names (numpy arrays; norm3 and downsample.1 hold the same values)."""
    shape, iters = RAFT_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 31803)
    B, _, H, W = shape
    coarse = rng.uniform(40.0, 215.0, (B, 3, H // 8, W // 8))
    image1 = np.kron(coarse, np.ones((8, 8))) + rng.normal(0.0, 8.0, shape)
    image2 = np.roll(image1, 2, axis=3) + rng.normal(0.0, 4.0, shape)
    image1, image2 = (np.clip(a, 0.0, 255.0).astype(np.float32) for a in (image1, image2))
    state = {}
    for prefix, norm, dim in (("fnet.", "instance", 256), ("cnet.", "batch", 256)):
        weights, biases, norms = encoder_parameters(rng, dim)
        for n, w, b in zip(PARAMETERS, weights, biases):
            state[f"{prefix}{n}.weight"], state[f"{prefix}{n}.bias"] = w, b
        if norm == "batch":
            for n, four in zip(NORMS, norms):
                names = [n] + ([n.replace("norm3", "downsample.1")] if n.endswith("norm3") else [])
                for m in names:
                    for v, a in zip(NORM_VECTORS, four):
                        state[f"{prefix}{m}.{v}"] = a
                    state[f"{prefix}{m}.num_batches_tracked"] = np.array(7, np.int64)
    for n, out, cin, k in bc.LAYERS:
        w, b = bc._conv_parameters(rng, out, cin, k)
        state[f"update_block.{n}.weight"], state[f"update_block.{n}.bias"] = w, b
    state = {k: state[k] for k in RAFT_STATE_DICT_KEYS}
    M = B * (H // 8) * (W // 8)
    low = np.sort(rng.choice(M, MAX_SAMPLES, replace=False)).astype(np.int64)
    up = np.sort(rng.choice(B * H * W, 4 * MAX_SAMPLES, replace=False)).astype(np.int64)
    return {"name": name, "image1": image1, "image2": image2, "iters": iters, "state": state, "samples_low": low, "samples_up": up}


def input_digest(case):
    hsh = hashlib.sha256()
    arrays = {k: v for k, v in case.items() if isinstance(v, np.ndarray)}
    for key in ("weights", "biases"):
        for i, a in enumerate(case.get(key, ())):
            arrays[f"{key}{i:02d}"] = a
    for i, four in enumerate(case.get("norms") or ()):
        for j, a in enumerate(four):
            arrays[f"norms{i:02d}_{j}"] = a
    for j, a in enumerate(case.get("norm") or ()):
        arrays[f"norm_{j}"] = a
    for k, a in (case.get("state") or {}).items():
        arrays["state." + k] = a
    for key in sorted(arrays):
        v = arrays[key]
        hsh.update(key.encode())
        hsh.update(str(v.dtype).encode())
        hsh.update(str(v.shape).encode())
        hsh.update(np.ascontiguousarray(v).tobytes())
    return hsh.hexdigest()


def sample_view(out, samples):
    """out [B, C, H, W] -> [len(samples), C]: the stored pixels' channels."""
    B, C, H, W = out.shape
    return out.transpose(0, 2, 3, 1).reshape(B * H * W, C)[samples]
