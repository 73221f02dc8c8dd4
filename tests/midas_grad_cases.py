"""Seeded inputs of the tests of the MiDaS decoder's backward operators (robust_cvd_amd/csrc/cvd_midas_grad.h;
tests/test_midas_grad_reference.py, tests/test_gpu_midas_grad.py, tests/golden/reference_py/make_midas_grad_golden.py).

numpy's generator, as tests/midas_cases.py.  Weights U(+-1/sqrt(fan_in)); the output gradient gy, the convolution's input x, the addend
and the mask tensor N(0, 1) with the border pixels of every image scaled by 3, so that a halo leaked from a neighbouring row or image
shows.  The masks of these operator cases are GIVEN f32 tensors, so they are exact in any arithmetic: no tie can flip them.  The
planted cases have small-integer gy, x, weights and addends: every gradient is an exact integer in any order of summation, so a wrong
tap, a wrong padding or a lost slice is an integer error."""
import hashlib

import numpy as np

from tests import midas_cases as mc
from tests import raftblock_cases as bc

MAX_SAMPLES = 16

#  name               (in, out, k, (B, H, W), addend, mask, relu_in, forced split or 0)
CONV_GRAD_CASES = {
    "g256_3x5":          (256, 256, 3, (1, 3, 5), True, True, True, 0),        # dead lanes; masked + addend
    "g256_9x9b2":        (256, 256, 3, (2, 9, 9), False, True, True, 0),       # tiles straddle rows and images; 162 pixels against the chain of 256
    "g2048_1x1":         (2048, 256, 3, (1, 1, 1), False, False, False, 0),    # only the centre tap's weight gradients are non-zero
    "g2048_2x3":         (2048, 256, 3, (1, 2, 3), False, False, False, 0),
    "g256_128_6x10":     (256, 128, 3, (1, 6, 10), False, False, False, 0),
    "g20_5x7":           (20, 20, 3, (1, 5, 7), True, False, True, 0),         # rows of 180 floats, ragged last chunk
    "g21_19_5x7b2":      (21, 19, 3, (2, 5, 7), True, True, True, 0),          # scalar weight loads, ragged channels both ways
    "g64_24x40b3":       (64, 64, 3, (3, 24, 40), False, True, True, 0),       # 2880 pixels: the weight gradient splits by the rule
    "k1_40_24_5x7b2":    (40, 24, 1, (2, 5, 7), True, True, False, 0),         # the 1 x 1 filter
    "k1_512_70_2x3":     (512, 70, 1, (1, 2, 3), False, False, True, 0),
    "planted_4x5b2":     (72, 40, 3, (2, 4, 5), True, True, True, 3),          # forced split 3; exact
    "planted_12x16b2":   (72, 40, 3, (2, 12, 16), True, True, True, 3),        # 384 pixels: two chains, so the weight gradient does split
}

UPSAMPLE_GRAD_CASES = dict(mc.UPSAMPLE_CASES)            # the forward's ten: name -> (input shape, aligned)


#  name -> ((B, H, W), non_negative, seed): the masks of these cases come from COMPUTED tensors (output_conv.2's result and the head's
#  output before its last ReLU), so the seeds are chosen such that no such value of the float64 restatement lies within its forward
#  bar of zero and torch's f32 signs agree with the f64 signs everywhere (tests/test_midas_grad_reference.py asserts both)
HEAD_GRAD_CASES = {"8x12": ((1, 8, 12), True, 0), "8x12_signed": ((1, 8, 12), False, 0), "5x7b2": ((2, 5, 7), True, 0),
                   "5x7b2_signed": ((2, 5, 7), False, 0)}
HEAD_PARAMETERS = ("weight2", "bias2", "weight4", "bias4")


def _normal(rng, shape):
    return bc._scale_border(rng.normal(0.0, 1.0, shape).astype(np.float32))


def _flat_samples(rng, size):
    if size <= MAX_SAMPLES:
        return np.arange(size, dtype=np.int64)
    return np.sort(np.r_[[0, size - 1], rng.choice(np.arange(1, size - 1), MAX_SAMPLES - 2, replace=False)]).astype(np.int64)


def make_conv_grad_case(name):
    cin, cout, k, (B, H, W), with_add, with_mask, relu_in, split = CONV_GRAD_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 32100)
    weight, _bias = bc._conv_parameters(rng, cout, cin, k)
    gy = _normal(rng, (B, cout, H, W))
    x = _normal(rng, (B, cin, H, W))
    add = _normal(rng, (B, cin, H, W))
    mask = _normal(rng, (B, cin, H, W))
    if name.startswith("planted"):
        weight = rng.integers(-2, 3, weight.shape).astype(np.float32)
        gy, x, add, mask = (rng.integers(-3, 4, v.shape).astype(np.float32) for v in (gy, x, add, mask))
    return {"name": name, "gy": gy, "x": x, "weight": weight, "k": k, "add": add if with_add else None, "mask": mask if with_mask else None,
            "relu_in": relu_in, "split": split,
            "samples": {"gx": _flat_samples(rng, x.size), "gw": _flat_samples(rng, weight.size), "gb": _flat_samples(rng, cout)}}


def make_upsample_grad_case(name):
    (B, Cn, H, W), aligned = UPSAMPLE_GRAD_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 32101)
    return {"name": name, "gy": rng.normal(0.0, 1.0, (B, Cn, 2 * H, 2 * W)).astype(np.float32), "align_corners": aligned,
            "samples": {"gx": _flat_samples(rng, B * Cn * H * W)}}


def make_head_grad_case(name):
    (B, H, W), non_negative, seed = HEAD_GRAD_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 32102 + 1000 * seed)
    weight2, bias2 = bc._conv_parameters(rng, mc.HEAD_MID, 128, 3)
    weight4, bias4 = bc._conv_parameters(rng, 1, mc.HEAD_MID, 1)
    bias4[0] = -0.05              # (with weights of both signs: some outputs are negative before the last ReLU)
    x = _normal(rng, (B, 128, H, W))
    gy = _normal(rng, (B, 1, H, W))[:, 0]
    samples = {"gx": _flat_samples(rng, x.size), "gw2": _flat_samples(rng, weight2.size), "gb2": _flat_samples(rng, mc.HEAD_MID),
               "gw4": _flat_samples(rng, mc.HEAD_MID), "gb4": _flat_samples(rng, 1)}
    return {"name": name, "gy": gy, "x": x, "weight2": weight2, "bias2": bias2, "weight4": weight4, "bias4": bias4,
            "non_negative": non_negative, "samples": samples}


# ---- small whole decoders: features 16 over a stub backbone to 16 / 21 / 40 / 72 channels (one non-zero power-of-two weight per
# output channel, as tests/midas_cases.py: the feature maps are exact in any arithmetic).  Their masks are computed tensors: the
# seeds are chosen for the tie condition.   name -> (image shape, non_negative, seed)
SMALL_FEATURES = 16
SMALL_CHANNELS = (16, 21, 40, 72)
SMALL_STUB_LAYERS = ((3, 16, 4), (16, 21, 2), (21, 40, 2), (40, 72, 2))
SMALL_DECODER_CASES = {"s16_32x32": ((1, 3, 32, 32), True, 0), "s16_64x32b2": ((2, 3, 64, 32), True, 0)}


def small_stub_weight(layer, entry):
    cin, cout, k = SMALL_STUB_LAYERS[layer]
    index, value = entry
    w = np.zeros((cout, cin * k * k), np.float32)
    w[np.arange(cout), index] = value
    return w.reshape(cout, cin, k, k)


def small_stub_maps(images, stub):
    maps, x = [], images
    for (cin, cout, k), (index, value) in zip(SMALL_STUB_LAYERS, stub):
        B, Cn, H, W = x.shape
        patches = x.reshape(B, cin, H // k, k, W // k, k).transpose(0, 2, 4, 1, 3, 5).reshape(B, H // k, W // k, cin * k * k)
        x = np.ascontiguousarray((patches[..., index] * value).transpose(0, 3, 1, 2))
        maps.append(x)
    return maps


def Feed(leaf):
    """A backbone stage (torch module) that returns the stored feature map, whatever it is given: with the four maps as leaves their
    .grad is the decoder's hand-over alone.  torch is imported when this is called."""
    import torch

    class _Feed(torch.nn.Module):
        def forward(self, _x):
            return leaf
    return _Feed()


def make_small_decoder_case(name):
    shape, non_negative, seed = SMALL_DECODER_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 32104 + 1000 * seed)
    stub = []
    for cin, cout, k in SMALL_STUB_LAYERS:
        stub.append((rng.integers(0, cin * k * k, cout).astype(np.int64),
                     (rng.choice([-1.0, 1.0], cout) * rng.choice([0.5, 1.0, 2.0], cout)).astype(np.float32)))
    params = {}
    for layer in mc.STATE_DICT_LAYERS:
        o, c, k, _ = mc.weight_shape(layer, SMALL_FEATURES, SMALL_CHANNELS)
        w, b = bc._conv_parameters(rng, o, c, k)
        params[layer] = (w, b if mc.has_bias(layer) else None)
    params["output_conv.4"][1][0] = 0.3
    images = rng.normal(0.0, 1.0, shape).astype(np.float32)
    B, _, H, W = shape
    gy = _normal(rng, (B, 1, H, W))[:, 0]
    weights = [params[n][0] for n in mc.PARAMETERS]
    biases = [params[n][1] for n in mc.PARAMETERS if mc.has_bias(n)]
    maps = small_stub_maps(images, stub)
    samples = {f"gw{i:02d}": _flat_samples(rng, w.size) for i, w in enumerate(weights)}
    samples.update({f"gb{i:02d}": _flat_samples(rng, b.size) for i, b in enumerate(biases)})
    samples.update({f"gm{k}": _flat_samples(rng, m.size) for k, m in enumerate(maps)})
    return {"name": name, "features": SMALL_FEATURES, "images": images, "stub": stub, "params": params, "non_negative": non_negative,
            "maps": maps, "weights": weights, "biases": biases, "gy": gy, "samples": samples}


def input_digest(case):
    hsh = hashlib.sha256()
    for key in sorted(k for k, v in case.items() if isinstance(v, np.ndarray)):
        v = case[key]
        hsh.update(key.encode())
        hsh.update(str(v.dtype).encode())
        hsh.update(str(v.shape).encode())
        hsh.update(np.ascontiguousarray(v).tobytes())
    for key in ("weights", "biases", "maps"):
        for i, v in enumerate(case.get(key, ())):
            hsh.update(f"{key}{i:02d}".encode())
            hsh.update(np.ascontiguousarray(v).tobytes())
    for key in ("relu_in", "align_corners", "non_negative"):
        if key in case:
            hsh.update(f"{key}={bool(case[key])}".encode())
    for key in sorted(case["samples"]):
        hsh.update(key.encode())
        hsh.update(case["samples"][key].tobytes())
    return hsh.hexdigest()
