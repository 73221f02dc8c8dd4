"""Seeded inputs of the ResNeXt backbone tests (robust_cvd_amd/csrc/cvd_resnext.h; tests/test_resnext_reference.py,
tests/test_gpu_resnext.py, tests/resnext_torch_child.py, tests/golden/reference_py/make_resnext_golden.py).

numpy's generator, not torch's.  Weights are He-scaled, U(+-sqrt(6 / fan_in)), so a ReLU network keeps its scale from layer to
layer; a batch norm's weight is U(0.5, 1.5) -- U(0.2, 0.5) for a block's LAST norm (bn3), so the residual stream of 33 blocks stays
within a few units --, its bias and running mean N(0, 0.1), its running variance U(0.5, 1.5).  Inputs are N(0, 1) with the border
pixels of every image scaled by 3, so that a halo leaked from a neighbouring row or image shows.  The planted cases have
small-integer weights and inputs and no norm: their result is exact in any order of summation, so a wrong tap, a wrong padding, a
wrong group or a lost slice of K is an integer error.

The architecture (conv_table, state_dict_keys) is written out here from torchvision's ResNet / Bottleneck (v1.5) and the reference's
monodepth/midas_v2/blocks.py:22-31, not imported from the package, so the tests pin the package's lists."""
import hashlib

import numpy as np

from tests import midas_cases as mc
from tests import raftblock_cases as bc

EPS = 1e-5
MAX_SAMPLES = 16
MAP_SAMPLES = 4                      # pixels stored per feature map of a backbone case (up to 2048 channels each)
GROUP_WIDTHS = (8, 16, 32, 64)
REAL = ((3, 4, 23, 3), 32, 8)        # ResNeXt-101 32x8d
SMALL = ((2, 1, 2, 1), 4, 8)         # channels per group 8, 16, 32, 64 with 4 groups


def conv_table(blocks, groups, width_per_group):
    """[(torchvision conv name, torchvision norm name, MidasNet.pretrained conv key, norm key, weight shape, stride, groups,
    last norm of a block)] in the state dict's order."""
    table = [("conv1", "bn1", "layer1.0", "layer1.1", (64, 3, 7, 7), 2, 1, False)]
    inplanes = 64
    for stage in range(4):
        planes = 64 * 2 ** stage
        per_group = int(planes * (width_per_group / 64.0))
        width = per_group * groups
        for i in range(blocks[stage]):
            stride = 2 if (stage > 0 and i == 0) else 1
            tv = f"layer{stage + 1}.{i}"
            md = f"layer1.4.{i}" if stage == 0 else tv
            table.append((f"{tv}.conv1", f"{tv}.bn1", f"{md}.conv1", f"{md}.bn1", (width, inplanes, 1, 1), 1, 1, False))
            table.append((f"{tv}.conv2", f"{tv}.bn2", f"{md}.conv2", f"{md}.bn2", (width, per_group, 3, 3), stride, groups, False))
            table.append((f"{tv}.conv3", f"{tv}.bn3", f"{md}.conv3", f"{md}.bn3", (4 * planes, width, 1, 1), 1, 1, True))
            if stride != 1 or inplanes != 4 * planes:
                table.append((f"{tv}.downsample.0", f"{tv}.downsample.1", f"{md}.downsample.0", f"{md}.downsample.1",
                              (4 * planes, inplanes, 1, 1), stride, 1, False))
            inplanes = 4 * planes
    return table


NORM_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def state_dict_keys(blocks, groups, width_per_group, prefix="pretrained."):
    """[(key, shape)] of the backbone under the reference's MidasNet, in its order."""
    out = []
    for _tv, _tvn, key, norm, shape, _s, _g, _last in conv_table(blocks, groups, width_per_group):
        out.append((prefix + key + ".weight", shape))
        out.extend((f"{prefix}{norm}.{v}", () if v == "num_batches_tracked" else (shape[0],)) for v in NORM_KEYS)
    return out


def he_weight(rng, shape):
    bound = np.sqrt(6.0 / float(shape[1] * shape[2] * shape[3]))
    return rng.uniform(-bound, bound, shape).astype(np.float32)


def norm_vectors(rng, n, last=False):
    """(weight, bias, running_mean, running_var) of an eval batch norm."""
    lo, hi = (0.2, 0.5) if last else (0.5, 1.5)
    return [rng.uniform(lo, hi, n).astype(np.float32), rng.normal(0.0, 0.1, n).astype(np.float32),
            rng.normal(0.0, 0.1, n).astype(np.float32), rng.uniform(0.5, 1.5, n).astype(np.float32)]


def _normal(rng, shape):
    return bc._scale_border(rng.normal(0.0, 1.0, shape).astype(np.float32))


def out_size(n, stride):
    return (n - 1) // stride + 1


# ---- grouped 3 x 3 ------------------------------------------------------------------------------------------------------------------
#  name              (groups, channels per group, stride, (B, H, W), relu)
GROUPED_CASES = {
    "g32x8_s1_5x7":     (32, 8, 1, (1, 5, 7), True),
    "g32x8_s2_5x7b2":   (32, 8, 2, (2, 5, 7), True),        # odd sides at stride 2; a tile across images
    "g3x8_s1_1x1":      (3, 8, 1, (1, 1, 1), False),        # the window is all padding but the centre; G no power of two
    "g3x8_s2_1x1":      (3, 8, 2, (1, 1, 1), False),
    "g32x16_s2_4x6":    (32, 16, 2, (1, 4, 6), True),       # even sides at stride 2
    "g5x32_s1_3x5":     (5, 32, 1, (1, 3, 5), True),
    "g32x64_s2_2x3":    (32, 64, 2, (1, 2, 3), True),
    "g2x64_s1_9x9b2":   (2, 64, 1, (2, 9, 9), False),       # 162 pixels
    "planted_g4x8_s2_4x5b2": (4, 8, 2, (2, 4, 5), False),   # exact
}


def make_grouped_case(name):
    G, cg, stride, (B, H, W), relu = GROUPED_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 32000)
    weight = he_weight(rng, (G * cg, cg, 3, 3))
    x = _normal(rng, (B, G * cg, H, W))
    norm = norm_vectors(rng, G * cg)
    if name.startswith("planted"):
        weight = rng.integers(-2, 3, weight.shape).astype(np.float32)
        x = rng.integers(-3, 4, x.shape).astype(np.float32)
        norm = None
    return {"name": name, "x": x, "weight": weight, "norm": norm, "stride": stride, "groups": G, "relu": relu,
            "samples": bc._samples(rng, B, out_size(H, stride), out_size(W, stride), MAX_SAMPLES)}


# ---- max pool -----------------------------------------------------------------------------------------------------------------------
POOL_CASES = {"1x1": (2, 3, 1, 1), "1x7": (2, 3, 1, 7), "5x1": (2, 3, 5, 1), "7x9": (2, 3, 7, 9), "6x10": (2, 3, 6, 10),
              "negative_7x9": (2, 3, 7, 9)}


def make_pool_case(name):
    shape = POOL_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 32001)
    x = rng.normal(0.0, 1.0, shape).astype(np.float32)
    if name.startswith("negative"):
        x[1] = -np.abs(x[1]) - np.float32(0.5)            # an all-negative image: a zero padding would show
    B, _, H, W = shape
    return {"name": name, "x": x, "samples": bc._samples(rng, B, out_size(H, 2), out_size(W, 2), MAX_SAMPLES)}


# ---- dense convolutions -------------------------------------------------------------------------------------------------------------
# form -> (norm, relu, residual): the combinations the backbone uses, and none at all
FORMS = {"conv1": (True, True, False), "conv3": (True, False, True), "down": (True, False, False), "bare": (False, False, False)}
#  name                 (in, out, k, stride, (B, H, W), form)
CONV_CASES = {
    "stem_9x11":         (3, 64, 7, 2, (1, 9, 11), "conv1"),
    "stem_8x8b2":        (3, 64, 7, 2, (2, 8, 8), "conv1"),
    "k1_s1_conv1":       (40, 24, 1, 1, (2, 5, 7), "conv1"),
    "k1_s1_conv3":       (40, 70, 1, 1, (2, 5, 7), "conv3"),
    "k1_s1_down":        (64, 256, 1, 1, (2, 5, 7), "down"),
    "k1_s2_down":        (40, 70, 1, 2, (2, 5, 7), "down"),
    "k1_s2_odd":         (21, 19, 1, 2, (2, 5, 7), "conv1"),     # rows of 21 floats: scalar weight loads, ragged channels
    "k1_2048_512_1x1":   (2048, 512, 1, 1, (1, 1, 1), "conv1"),  # S = 8
    "k1_2048_512_2x3":   (2048, 512, 1, 1, (1, 2, 3), "conv3"),
    "k1_1024_2048_s2":   (1024, 2048, 1, 2, (1, 3, 4), "down"),  # S = 4 at stride 2
    "planted_512_40":    (512, 40, 1, 1, (2, 2, 3), "bare"),     # S = 2; exact
}
SPLIT_CASES = ("k1_2048_512_1x1", "k1_2048_512_2x3", "k1_1024_2048_s2")
EXPECTED_SPLIT = {"k1_2048_512_1x1": 8, "k1_2048_512_2x3": 8, "k1_1024_2048_s2": 4, "planted_512_40": 2, "stem_9x11": 1, "k1_s1_conv1": 1}


def make_conv_case(name):
    cin, cout, k, stride, (B, H, W), form = CONV_CASES[name]
    with_norm, relu, with_residual = FORMS[form]
    rng = np.random.default_rng(sum(name.encode()) + 32002)
    weight = he_weight(rng, (cout, cin, k, k))
    x = _normal(rng, (B, cin, H, W))
    Ho, Wo = out_size(H, stride), out_size(W, stride)
    residual = np.maximum(_normal(rng, (B, cout, Ho, Wo)), np.float32(0.0))       # (a block's input is rectified)
    norm = norm_vectors(rng, cout, last=form == "conv3")
    if name.startswith("planted"):
        weight = rng.integers(-2, 3, weight.shape).astype(np.float32)
        x = rng.integers(-3, 4, x.shape).astype(np.float32)
    return {"name": name, "x": x, "weight": weight, "norm": norm if with_norm else None, "stride": stride, "relu": relu,
            "residual": residual if with_residual else None, "samples": bc._samples(rng, B, Ho, Wo, MAX_SAMPLES)}


# ---- bottlenecks --------------------------------------------------------------------------------------------------------------------
#  name             (inplanes, planes, stride, groups, width_per_group, (B, H, W))
BLOCK_CASES = {
    "layer1_0":       (64, 64, 1, 4, 8, (1, 5, 7)),          # 64 -> 32 -> 256, downsample at stride 1
    "stride2":        (256, 128, 2, 4, 8, (2, 5, 7)),        # 256 -> 64 -> 512, downsample at stride 2
    "identity":       (256, 64, 1, 4, 8, (1, 6, 6)),         # no downsample
}


def block_parameters(rng, inplanes, planes, stride, groups, width_per_group):
    """[(weight, norm)] for conv1, conv2, conv3 and, where torchvision builds one, downsample.0."""
    per_group = int(planes * (width_per_group / 64.0))
    width = per_group * groups
    shapes = [(width, inplanes, 1, 1), (width, per_group, 3, 3), (4 * planes, width, 1, 1)]
    if stride != 1 or inplanes != 4 * planes:
        shapes.append((4 * planes, inplanes, 1, 1))
    return [(he_weight(rng, s), norm_vectors(rng, s[0], last=i == 2)) for i, s in enumerate(shapes)]


def make_block_case(name):
    inplanes, planes, stride, groups, wpg, (B, H, W) = BLOCK_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 32003)
    params = block_parameters(rng, inplanes, planes, stride, groups, wpg)
    x = np.maximum(_normal(rng, (B, inplanes, H, W)), np.float32(0.0))
    return {"name": name, "x": x, "params": params, "stride": stride, "groups": groups,
            "samples": bc._samples(rng, B, out_size(H, stride), out_size(W, stride), MAX_SAMPLES)}


# ---- whole backbones and whole networks ---------------------------------------------------------------------------------------------
#  name -> ((blocks, groups, width_per_group), image shape)
BACKBONE_CASES = {
    "small_32x32":    (SMALL, (1, 3, 32, 32)),
    "small_64x96b2":  (SMALL, (2, 3, 64, 96)),
    "real_32x64":     (REAL, (1, 3, 32, 64)),                # weights from the seed, not stored
}
#  name -> ((blocks, groups, width_per_group), features, image shape, non_negative)
NET_CASES = {"small_f64_64x64": (SMALL, 64, (1, 3, 64, 64), False)}      # (signed: every output pixel carries information)


def backbone_parameters(rng, blocks, groups, width_per_group):
    """[(weight, norm)] in conv_table's order."""
    return [(he_weight(rng, shape), norm_vectors(rng, shape[0], last=last))
            for _a, _b, _c, _d, shape, _s, _g, last in conv_table(blocks, groups, width_per_group)]


def _map_samples(rng, M):
    """The first and the last pixel of the batch and two drawn ones (all of them where the map has no more)."""
    if M <= MAP_SAMPLES:
        return np.arange(M, dtype=np.int64)
    return np.sort(np.r_[0, M - 1, rng.choice(np.arange(1, M - 1), MAP_SAMPLES - 2, replace=False)]).astype(np.int64)


def make_backbone_case(name):
    (blocks, groups, wpg), shape = BACKBONE_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 32004)
    params = backbone_parameters(rng, blocks, groups, wpg)
    B, _, H, W = shape
    images = rng.normal(0.0, 1.0, shape).astype(np.float32)
    return {"name": name, "blocks": blocks, "groups": groups, "width_per_group": wpg, "images": images, "params": params,
            "samples": [_map_samples(rng, B * (H >> (k + 2)) * (W >> (k + 2))) for k in range(4)]}


def make_net_case(name):
    (blocks, groups, wpg), features, shape, non_negative = NET_CASES[name]
    rng = np.random.default_rng(sum(name.encode()) + 32005)
    params = backbone_parameters(rng, blocks, groups, wpg)
    decoder = mc.decoder_parameters(rng, features)
    B, _, H, W = shape
    return {"name": name, "blocks": blocks, "groups": groups, "width_per_group": wpg, "features": features, "non_negative": non_negative,
            "images": rng.normal(0.0, 1.0, shape).astype(np.float32), "params": params, "decoder": decoder,
            "samples": bc._samples(rng, B, H, W, 4 * MAX_SAMPLES)}


def input_digest(case):
    hsh = hashlib.sha256()

    def feed(key, v):
        hsh.update(key.encode())
        hsh.update(str(v.dtype).encode())
        hsh.update(str(v.shape).encode())
        hsh.update(np.ascontiguousarray(v).tobytes())
    for key in sorted(k for k, v in case.items() if isinstance(v, np.ndarray)):
        feed(key, case[key])
    for i, a in enumerate(case.get("norm") or ()):
        feed(f"norm{i}", a)
    if isinstance(case.get("params"), list):
        for i, (w, four) in enumerate(case["params"]):
            feed(f"params{i:03d}.weight", w)
            for j, a in enumerate(four):
                feed(f"params{i:03d}.norm{j}", a)
    for k, (w, b) in sorted((case.get("decoder") or {}).items()):
        feed("decoder." + k + ".weight", w)
        if b is not None:
            feed("decoder." + k + ".bias", b)
    for key in ("stride", "groups", "relu", "blocks", "width_per_group", "features", "non_negative"):
        if key in case:
            hsh.update(f"{key}={case[key]}".encode())
    return hsh.hexdigest()


sample_view = mc.sample_view
