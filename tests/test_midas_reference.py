"""The float64 restatement of the MiDaS decoder (tests/midas_reference.py) against the fixture minted from the reference's own classes
(tests/golden/reference_py/midas_golden.npz), and where the reference checkout is present against the live classes; the split rule
of csrc/cvd_midas.h; the state-dict keys.  No GPU."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from robust_cvd_amd import api
from tests import midas_cases as mc
from tests import midas_reference as mr
from tests.codegen_util import CSRC, HIPCC, ROOT

FAMILIES = (("conv", mc.CONV_CASES, mc.make_conv_case, mr.conv_case), ("upsample", mc.UPSAMPLE_CASES, mc.make_upsample_case, None),
            ("head", mc.HEAD_CASES, mc.make_head_case, mr.head_case), ("unit", mc.UNIT_CASES, mc.make_unit_case, mr.unit_case),
            ("fusion", mc.FUSION_CASES, mc.make_fusion_case, mr.fusion_case), ("decoder", mc.DECODER_CASES, mc.make_decoder_case, mr.decoder_case))


@pytest.fixture(scope="module")
def golden():
    return np.load(mr.GOLDEN)


def restate(family, case):
    if family == "upsample":
        return mr.upsample2x(case["x"], case["align_corners"])
    return dict((f[0], f[3]) for f in FAMILIES)[family](case)


@pytest.mark.parametrize("family,name", [(f[0], n) for f in FAMILIES for n in f[1]])
def test_restatement_lies_within_delta_of_the_reference(golden, family, name):
    case = dict((f[0], f[2]) for f in FAMILIES)[family](name)
    key = f"{family}/{name}"
    assert mc.input_digest(case) == golden[f"{key}/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    want = restate(family, case)
    delta, scale = float(golden[f"{key}/out_delta"]), float(golden[f"{key}/out_scale"])
    assert np.abs(want).max() == pytest.approx(scale, rel=1e-12)
    assert delta <= 64 * mr.EPS32 * max(scale, 1.0), "the reference's f32 arithmetic lies far from the restatement"
    assert np.abs(mc.sample_view(want, case["samples"]) - golden[f"{key}/out"]).max() <= delta


def test_the_unit_fixture_tells_the_in_place_relu_from_the_plain_form(golden):
    """conv2(relu(conv1(relu(x)))) + relu(x) is what the reference computes (its nn.ReLU is in place); `... + x` is off by the
    negative part of x, far above the bar."""
    for family, make, restated in (("unit", mc.make_unit_case, mr.unit_case), ("fusion", mc.make_fusion_case, mr.fusion_case)):
        for name in dict((f[0], f[1]) for f in FAMILIES)[family]:
            case = make(name)
            key = f"{family}/{name}"
            stored = golden[f"{key}/out"]
            bar = mr.bar(golden[f"{key}/out_delta"], golden[f"{key}/out_scale"])
            assert min(float(case[k].min()) for k in ("x", "x0", "x1") if k in case) < -3.0        # a large negative part
            assert np.abs(mc.sample_view(restated(case), case["samples"]) - stored).max() <= bar
            plain = np.abs(mc.sample_view(restated(case, inplace=False), case["samples"]) - stored).max()
            assert plain > 1e4 * bar and plain > 1.0, (key, plain, bar)


def test_the_decoder_fixture_tells_the_in_place_relu_too(golden):
    case = mc.make_decoder_case("f64_64x64")
    key = "decoder/f64_64x64"
    bar = mr.bar(golden[f"{key}/out_delta"], golden[f"{key}/out_scale"])
    plain = mr.decoder(case["maps"], case["params"], case["non_negative"], inplace=False)
    assert np.abs(mc.sample_view(plain, case["samples"]) - golden[f"{key}/out"]).max() > 100 * bar


def test_restatement_against_the_live_classes(golden):
    """The reference's own ResidualConvUnit and MidasNet (over the stub backbone), run here: the stored values are theirs, and the
    restatement lies within the bar of them over ALL pixels."""
    reference = mr.load_reference()
    if reference is None:
        pytest.skip("the reference checkout (or torch) is not available here")
    import torch
    from tests.golden.reference_py import make_midas_golden as mint
    blocks = reference[0]
    with torch.no_grad():
        case = mc.make_unit_case("rcu_64_6x7")
        x = torch.from_numpy(case["x"].copy())
        live = mint.load_unit(blocks.ResidualConvUnit(64), case["weights"], case["biases"])(x).numpy()
        assert (x.numpy() == np.maximum(case["x"], 0.0)).all()          # the reference rectified its caller's tensor
        results = [("unit/rcu_64_6x7", case, live, mr.unit_case(case))]
        case = mc.make_decoder_case("f64_64x64")
        live = mr.reference_net(reference, case)(torch.from_numpy(case["images"])).numpy()
        results.append(("decoder/f64_64x64", case, live, mr.decoder_case(case)))
    for key, case, live, want in results:
        delta, scale = float(golden[f"{key}/out_delta"]), float(golden[f"{key}/out_scale"])
        assert np.abs(live - want).max() <= 4 * max(delta, mr.EPS32 * scale), key
        assert np.abs(mc.sample_view(live, case["samples"]) - golden[f"{key}/out"]).max() <= 4 * max(delta, mr.EPS32 * scale), key


def test_upsampling_a_single_pixel_gives_copies():
    x = np.array([[[[2.5]]]], np.float32)
    for aligned in (True, False):
        assert (mr.upsample2x(x, aligned) == 2.5).all() and mr.upsample2x(x, aligned).shape == (1, 1, 2, 2)


# (K, H W) of the decoder's layers at 384 x 224 frames -> S: layer4_rn, layer3_rn, layer2_rn, layer1_rn, refinenet4 .. refinenet1,
# output_conv.0
SPLITS_384x224 = (((2048 * 9, 84), 32), ((1024 * 9, 336), 8), ((512 * 9, 1344), 3), ((256 * 9, 5376), 1), ((256 * 9, 84), 8),
                  ((256 * 9, 336), 8), ((256 * 9, 1344), 3), ((256 * 9, 5376), 1), ((256 * 9, 21504), 1))


def test_the_split_rule_is_a_function_of_k_and_the_pixels_of_one_image():
    assert list(inspect.signature(api.midas_split).parameters) == ["K", "HW", "kernel_size"]
    for (K, HW), want in SPLITS_384x224:
        assert api.midas_split(K, HW) == want, (K, HW)
    for K in (9, 180, 189, 576, 2304, 4608, 9216, 18432, 36864):
        last = None
        for HW in (1, 6, 63, 64, 65, 84, 336, 1344, 4096, 4097, 5376, 100000):
            S = api.midas_split(K, HW)
            chains = -(-(-(-K // 72)) // 4)
            assert 1 <= S <= min(chains, api.MIDAS_MAX_SPLIT)
            assert last is None or S <= last           # more pixels never split further
            last = S
            # every slice is whole chains and none is empty
            ranges = api.midas_slice_channels(K // 9, 3, S)
            assert len(ranges) == S and ranges[0][0] == 0 and ranges[-1][1] == K // 9
            assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and all((c1 - c0) % 32 == 0 for c0, c1 in ranges[:-1])
        assert api.midas_split(K, 5000) == 1
    assert api.midas_split(512, 6, 1) == 2 and api.midas_split(40, 35, 1) == 1


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_python_rule_is_the_headers(tmp_path):
    """midasSplit of csrc/cvd_midas.h, compiled for the host, against api.midas_split."""
    points = [(K, HW, ks) for K in (9, 180, 189, 576, 2304, 9216, 18432, 36864) for HW in (1, 6, 64, 65, 84, 336, 1344, 4097, 5376) for ks in (3,)]
    points += [(K, HW, 1) for K in (32, 40, 256, 512, 2048, 8192) for HW in (1, 6, 84, 1344, 5376)]
    src = tmp_path / "split.hip"
    src.write_text(f'#include <cstdio>\n#include "{CSRC}/cvd_midas.h"\nint main() {{\n'
                   + "".join(f'  std::printf("%d\\n", cvd::midasSplit({K}ll, {HW}ll, {ks}));\n' for K, HW, ks in points) + "  return 0;\n}\n")
    exe = tmp_path / "split"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", str(exe), str(src)], check=True, capture_output=True, timeout=300)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [api.midas_split(K, HW, ks) for K, HW, ks in points]


def test_the_state_dict_keys_are_the_references(golden):
    keys = tuple(str(k) for k in golden["state_dict_keys"])
    assert len(keys) == 42 and keys == mc.STATE_DICT_KEYS == api.MIDAS_STATE_DICT_KEYS
    assert api.MIDAS_PARAMETERS == mc.PARAMETERS and len(api.MIDAS_PARAMETERS) == 21
    for name in mc.STATE_DICT_LAYERS:
        for features in (256, 64):
            assert api.midas_weight_shape(name, features) == mc.weight_shape(name, features)


def test_the_module_has_the_references_keys_and_never_fetches():
    """robust_cvd_amd.midas.MidasNet over a stub backbone, in a fresh process (torch is imported before the library there): the 42
    scratch.* keys in the reference's order, a strict load of a reference-shaped state dict, an ImportError that names torchvision
    where it is missing, and no torch.hub anywhere in the package, the tests' helpers aside, or the tools."""
    code = (
        "import importlib.util, sys, torch\n"
        "from robust_cvd_amd import midas\n"
        "from tests import midas_cases as mc, midas_reference as mr\n"
        "case = mc.make_decoder_case('f64_64x64')\n"
        "net = midas.MidasNet(features=64, backbone=mr.stub_backbone(case['stub']))\n"
        "keys = [k for k in net.state_dict() if k.startswith('scratch.')]\n"
        "assert tuple(keys) == mc.STATE_DICT_KEYS, keys\n"
        "assert all(k.startswith(('scratch.', 'pretrained.')) for k in net.state_dict())\n"
        "sd = net.state_dict(); sd.update(mr.scratch_state_dict(case)); net.load_state_dict(sd, strict=True)\n"
        "if importlib.util.find_spec('torchvision') is None:\n"
        "    try:\n"
        "        midas.MidasNet()\n"
        "        raise SystemExit('no ImportError')\n"
        "    except ImportError as e:\n"
        "        assert 'torchvision' in str(e)\n"
        "print('midas module keys ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "midas module keys ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    for folder in ("robust_cvd_amd", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, folder)):
            for f in files:
                if f.endswith(".py"):
                    text = open(os.path.join(dirpath, f)).read()
                    assert "torch.hub" not in text and "hub.load" not in text, f
