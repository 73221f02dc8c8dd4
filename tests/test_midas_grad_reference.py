"""The float64 restatement of the MiDaS decoder layers' backward (tests/midas_grad_reference.py) against the fixture minted under
torch's autograd (tests/golden/reference_py/midas_grad_golden.npz), the adjoint identities of the three linear operators, and the
split rule of the weight gradient (csrc/cvd_midas_grad.h).  No GPU."""
import inspect
import os
import subprocess

import numpy as np
import pytest

from robust_cvd_amd import api
from tests import midas_grad_cases as gc
from tests import midas_grad_reference as gr
from tests import midas_reference as mr
from tests.codegen_util import CSRC, HIPCC

FAMILIES = (("conv", gc.CONV_GRAD_CASES, gc.make_conv_grad_case, gr.conv_grad_case),
            ("upsample", gc.UPSAMPLE_GRAD_CASES, gc.make_upsample_grad_case, gr.upsample_grad_case),
            ("head", gc.HEAD_GRAD_CASES, gc.make_head_grad_case, gr.head_grad_case),
            ("decoder", gc.SMALL_DECODER_CASES, gc.make_small_decoder_case, gr.decoder_grad_case))


@pytest.fixture(scope="module")
def golden():
    return np.load(gr.GOLDEN)


@pytest.mark.parametrize("family,name", [(f[0], n) for f in FAMILIES for n in f[1]])
def test_restatement_lies_within_delta_of_the_reference(golden, family, name):
    _f, _cases, make, restate = [f for f in FAMILIES if f[0] == family][0]
    case = make(name)
    key = f"{family}/{name}"
    assert gc.input_digest(case) == golden[f"{key}/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    for tensor, want in restate(case).items():
        delta, scale = float(golden[f"{key}/{tensor}_delta"]), float(golden[f"{key}/{tensor}_scale"])
        assert np.abs(want).max() == pytest.approx(scale, rel=1e-12)
        assert delta <= 64 * mr.EPS32 * max(scale, 1.0), "torch's f32 arithmetic lies far from the restatement"
        assert np.abs(want.reshape(-1)[case["samples"][tensor]] - golden[f"{key}/{tensor}"]).max() <= delta
        if name.startswith("planted"):
            assert delta == 0.0 and (want == np.round(want)).all()


@pytest.mark.parametrize("name", list(gc.HEAD_GRAD_CASES))
def test_the_head_cases_have_no_tie_at_a_relu(golden, name):
    """The tie condition of the cases whose masks come from computed tensors: no rectified pre-activation of the f64 restatement lies
    within that tensor's forward bar of zero, torch's f32 signs agree with the f64 signs everywhere (recorded at minting), and both
    masks have work.  No element is dropped to meet it: the seeds of tests/midas_grad_cases.py are chosen."""
    case = gc.make_head_grad_case(name)
    for tensor, value in zip(("t", "s"), gr.head_forward(case)):
        key = f"head/{name}/{tensor}"
        if tensor == "s" and not case["non_negative"]:
            continue                                  # the signed head does not rectify its output
        forward_bar = mr.bar(golden[key + "_delta"], golden[key + "_scale"])
        assert np.abs(value).min() > forward_bar, (key, np.abs(value).min(), forward_bar)
        assert bool(golden[key + "_signs_agree"]), key
        assert (value <= 0).any() and (value > 0).any(), key


@pytest.mark.parametrize("name", list(gc.SMALL_DECODER_CASES))
def test_the_small_decoder_cases_have_no_tie_at_a_relu(golden, name):
    """The same condition for every tensor a ReLU of the whole decoder reads -- the layerK_rn results, the units' conv1 results, the
    fusion sums, output_conv.2's result and the output --: 16 tensors, from the restatement and from the reference's own MidasNet
    (its f32 values were captured by hooks at minting)."""
    case = gc.make_small_decoder_case(name)
    tensors = gr.rectified(gr.decoder_forward(case))
    assert len(tensors) == 16
    for tensor, value in tensors.items():
        key = f"decoder/{name}/{tensor}"
        forward_bar = mr.bar(golden[key + "_delta"], golden[key + "_scale"])
        assert np.abs(value).min() > forward_bar, (key, np.abs(value).min(), forward_bar)
        assert bool(golden[key + "_signs_agree"]), key
        if tensor != "s":
            assert (value <= 0).any() and (value > 0).any(), key
    got = gr.decoder_grad_case(case)
    assert len(got) == 21 + 17 + 4 and api.midas_saved_shapes(1, 16, (8, 4, 2, 1), (8, 4, 2, 1))[14:] == [(1, 16, 16, 16), (1, 128, 16, 16)]
    assert len(api.midas_saved_shapes(2, 256, (56, 28, 14, 7), (96, 48, 24, 12))) == api.MIDAS_SAVED == 16
    assert api.midas_saved_shapes(2, 256, (56, 28, 14, 7), (96, 48, 24, 12))[4:8] == [(2, 256, 7, 12), (2, 256, 14, 24)] * 1 + [(2, 256, 14, 24)] * 2
    assert len(api.midas_backward_stages()) == 45 and len(api.midas_backward_stages(False)) == 41 <= api.MIDAS_BACKWARD_SLOTS


def test_only_the_centre_tap_sees_a_single_pixel():
    case = gc.make_conv_grad_case("g2048_1x1")
    gw, gb = gr.conv_grad_weight(case["gy"], case["x"], 3)
    off = np.ones((3, 3), bool)
    off[1, 1] = False
    assert (gw[:, :, off] == 0).all() and (gw[:, :, 1, 1] != 0).any()
    assert (gb == case["gy"][0, :, 0, 0]).all()


@pytest.mark.parametrize("name", ["planted_4x5b2", "planted_12x16b2"])
def test_the_convolution_gradients_are_the_adjoints_exactly(name):
    """<gy, conv(u, W)> = <dgrad(gy, W), u> and <gy, conv(X, V)> = <wgrad(gy, X), V> on small integers: exact in f64, and independent
    of torch."""
    case = gc.make_conv_grad_case(name)
    rng = np.random.default_rng(5)
    u = rng.integers(-3, 4, case["x"].shape).astype(np.float64)
    v = rng.integers(-2, 3, case["weight"].shape).astype(np.float64)
    gy = case["gy"].astype(np.float64)
    assert (gy * gr.conv_forward(u, case["weight"])).sum() == (gr.conv_grad_input(gy, case["weight"]) * u).sum()
    for relu_in in (False, True):
        gw, gb = gr.conv_grad_weight(gy, case["x"], case["k"], relu_in)
        assert (gy * gr.conv_forward(case["x"], v, relu_in)).sum() == (gw * v).sum()
        assert (gb == gy.sum(axis=(0, 2, 3))).all()


@pytest.mark.parametrize("shape", list(gc.mc.UPSAMPLE_SHAPES.values()))
def test_the_upsampling_gradient_is_the_adjoint(shape):
    """<gy, up(u)> = <up^T(gy), u> on small integers.  Exact in the half-pixel mode, whose weights are 1/4 and 3/4; in the aligned
    mode the weights are multiples of 1 / (2 n - 1), not dyadic, so the two sides agree to the rounding of f64 only."""
    B, Cn, H, W = shape
    rng = np.random.default_rng(6)
    u = rng.integers(-3, 4, shape).astype(np.float64)
    gy = rng.integers(-3, 4, (B, Cn, 2 * H, 2 * W)).astype(np.float64)
    for aligned in (False, True):
        left, right = (gy * mr.upsample2x(u, aligned)).sum(), (gr.upsample2x_grad(gy, aligned) * u).sum()
        if aligned:
            assert abs(left - right) <= 1e-13 * np.abs(gy).sum() * 3
        else:
            assert left == right
    if (H, W) == (1, 1):
        for aligned in (False, True):
            assert (gr.upsample2x_grad(gy, aligned)[..., 0, 0] == gy.sum(axis=(2, 3))).all()


# (B H W, N, Cin KS KS) of the decoder's layers at 384 x 224 frames -> S: layer4_rn at B = 1 and 8, refinenet1's units, output_conv.0,
# output_conv.2 at B = 1 and 8; and the test case that splits by the rule
WGRAD_SPLITS = (((84, 256, 18432), 1), ((672, 256, 18432), 1), ((5376, 256, 2304), 7), ((21504, 128, 2304), 14),
                ((86016, 32, 1152), 56), ((688128, 32, 1152), 56), ((2880, 64, 576), 12), ((40, 40, 648), 1), ((384, 40, 648), 2))


def test_the_wgrad_split_rule_is_a_function_of_the_three_gemm_sizes():
    assert list(inspect.signature(api.midas_wgrad_split).parameters) == ["pixels", "out_channels", "columns"]
    for (M, N, Q), want in WGRAD_SPLITS:
        assert api.midas_wgrad_split(M, N, Q) == want, (M, N, Q)
    for N, Q in ((32, 1152), (256, 2304), (256, 18432), (19, 189), (1, 1)):
        last = 0
        for M in (1, 255, 256, 257, 2880, 86016, 10 ** 7):
            S = api.midas_wgrad_split(M, N, Q)
            chains = -(-M // api.MIDAS_WGRAD_CHAIN)
            assert 1 <= S <= min(chains, api.MIDAS_WGRAD_MAX_SPLIT)
            per = -(-chains // S)
            assert (S - 1) * per < chains           # whole chains a slice, none empty
            assert S >= last                        # more pixels never split less
            last = S


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_python_rule_is_the_headers(tmp_path):
    """midasWgradSplit of csrc/cvd_midas_grad.h, compiled for the host, against api.midas_wgrad_split."""
    points = [(M, N, Q) for M in (1, 40, 162, 256, 257, 2880, 5376, 86016, 688128) for N, Q in ((32, 1152), (256, 2304), (256, 18432), (19, 189), (70, 512))]
    src = tmp_path / "split.hip"
    src.write_text(f'#include <cstdio>\n#include "{CSRC}/cvd_midas_grad.h"\nint main() {{\n'
                   + "".join(f'  std::printf("%d\\n", cvd::midasWgradSplit({M}ll, {N}ll, {Q}ll));\n' for M, N, Q in points) + "  return 0;\n}\n")
    exe = tmp_path / "split"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", str(exe), str(src)], check=True, capture_output=True, timeout=300)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [api.midas_wgrad_split(M, N, Q) for M, N, Q in points]


def test_the_shape_checks_refuse_before_any_device_work():
    for bad in (lambda: api.midas_check_conv_grad_input((1, 8, 4, 4), (8, 4, 2, 2)),                # filter size
                lambda: api.midas_check_conv_grad_input((1, 8, 4, 4), (7, 4, 3, 3)),                # channels
                lambda: api.midas_check_conv_grad_input((1, 8, 4, 4), (8, 4, 3, 3), add_shape=(1, 8, 4, 4)),
                lambda: api.midas_check_conv_grad_input((1, 8, 4, 4), (8, 4, 3, 3), mask_shape=(1, 4, 4, 5)),
                lambda: api.midas_check_conv_grad_input((1, 8, 4, 4), (8, 4, 3, 3), split=2),       # one chunk of K
                lambda: api.midas_check_conv_grad_input((0, 8, 4, 4), (8, 4, 3, 3)),
                lambda: api.midas_check_conv_grad_weight((1, 8, 4, 4), (1, 4, 4, 5), 3),
                lambda: api.midas_check_conv_grad_weight((1, 8, 4, 4), (1, 4, 4, 4), 2),
                lambda: api.midas_check_conv_grad_weight((1, 8, 4, 4), (1, 4, 4, 4), 3, split=129),
                lambda: api.midas_check_conv_grad_weight((1, 8, 4, 4), (1, 4, 4, 4), 3, split=-1),
                lambda: api.midas_check_upsample2x_grad((1, 2, 3, 4)),
                lambda: api.midas_check_upsample2x_grad((1, 2, 4))):
        with pytest.raises(ValueError):
            bad()
    assert api.midas_check_conv_grad_input((2, 8, 4, 5), (8, 4, 3, 3), (2, 4, 4, 5), (2, 4, 4, 5)) == (2, 4, 5, 4, 8, 3)
    assert api.midas_check_conv_grad_weight((2, 8, 4, 5), (2, 4, 4, 5), 1) == (2, 4, 5, 4, 8, 1)
    assert api.midas_check_upsample2x_grad((1, 2, 6, 4)) == (1, 2, 3, 2)
