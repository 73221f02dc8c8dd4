"""GPU checks of the MiDaS decoder kernels (robust_cvd_amd/csrc/cvd_midas.h) through the array paths
(Solver.midas_conv, midas_upsample2x, midas_head, midas_decoder) and, in a fresh process, through the torch drop-in
robust_cvd_amd.midas (tests/midas_torch_child.py).

Bar: |kernel - f64| <= 8 x max(delta, 2^-23 x scale) against the float64 restatement (tests/midas_reference.py), delta = the
REFERENCE's own f32 error against that restatement for the case, scale = the largest |output|, both read from the fixture
(tests/golden/reference_py/midas_golden.npz, minted on the CPU from the reference's own classes; never from these kernels); against
the reference's stored f32 values that bar + delta.  The factor 8 is the one the project's other f32 kernels carry."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from robust_cvd_amd import api
from tests import margins
from tests import midas_cases as mc
from tests import midas_reference as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    return api.Solver(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(mr.GOLDEN)


def run_conv(solver, case, split=0, **over):
    c = dict(case, **over)
    return solver.midas_conv(c["x"], c["weight"], c["bias"], relu_in=c["relu_in"], relu=c["relu"], a=c["a"], relu_a=c["relu_a"], b=c["b"],
                             split=split)


def run_head(solver, case, **over):
    c = dict(case, **over)
    return solver.midas_head(c["x"], c["weight2"], c["bias2"], c["weight4"], c["bias4"], non_negative=c["non_negative"])


def run_decoder(solver, case, maps=None):
    return solver.midas_decoder(case["maps"] if maps is None else maps, case["weights"], case["biases"], non_negative=case["non_negative"])


def unit(solver, x, weights, biases, other=None):
    """A ResidualConvUnit as the library chains it: conv1 behind the input ReLU, conv2 + relu(x) (+ the other path)."""
    t = solver.midas_conv(x, weights[0], biases[0], relu_in=True)
    return solver.midas_conv(t, weights[1], biases[1], relu_in=True, a=x, relu_a=True, b=other)


def chain(solver, case):
    """The decoder's stages one by one through midas_conv, midas_upsample2x and midas_head, as cvd_midas_decoder_device chains them."""
    p = case["params"]
    rn = [solver.midas_conv(m, p[f"layer{k + 1}_rn"][0]) for k, m in enumerate(case["maps"])]
    path = None
    for k in (4, 3, 2, 1):
        w = [p[f"refinenet{k}.resConfUnit{u}.conv{c}"] for u in (1, 2) for c in (1, 2)]
        out = rn[k - 1]
        if path is not None:
            out = unit(solver, rn[k - 1], [w[0][0], w[1][0]], [w[0][1], w[1][1]], other=path)
        path = solver.midas_upsample2x(unit(solver, out, [w[2][0], w[3][0]], [w[2][1], w[3][1]]), align_corners=True)
    y = solver.midas_upsample2x(solver.midas_conv(path, *p["output_conv.0"]), align_corners=False)
    return solver.midas_head(y, *p["output_conv.2"], *p["output_conv.4"], non_negative=case["non_negative"])


@pytest.fixture(scope="module")
def conv_results(solver):
    """Per single-convolution case: (inputs, f64 restatement, kernel output): computed once, shared."""
    out = {}
    for name in mc.CONV_CASES:
        case = mc.make_conv_case(name)
        out[name] = (case, mr.conv_case(case), run_conv(solver, case))
    return out


@pytest.fixture(scope="module")
def upsample_results(solver):
    out = {}
    for name in mc.UPSAMPLE_CASES:
        case = mc.make_upsample_case(name)
        out[name] = (case, mr.upsample2x(case["x"], case["align_corners"]), solver.midas_upsample2x(case["x"], case["align_corners"]))
    return out


@pytest.fixture(scope="module")
def head_results(solver):
    out = {}
    for name in mc.HEAD_CASES:
        case = mc.make_head_case(name)
        out[name] = (case, mr.head_case(case), run_head(solver, case))
    return out


@pytest.fixture(scope="module")
def decoder_results(solver):
    out = {}
    for name in mc.DECODER_CASES:
        case = mc.make_decoder_case(name)
        out[name] = (case, mr.decoder_case(case), run_decoder(solver, case))
    return out


def check(label, key, golden, case, got, want):
    assert mc.input_digest(case) == golden[f"{key}/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    delta = float(golden[f"{key}/out_delta"])
    bar = mr.bar(delta, golden[f"{key}/out_scale"])
    err = np.abs(got - want).max()
    print(f"{key}: max |kernel - f64| {err:.3e}, bar {bar:.3e}, share {err / bar if bar else 0.0:.3f} (reference's own delta {delta:.3e})")
    margins.below(label, err, bar)
    margins.below(f"{label} vs reference", np.abs(mc.sample_view(got, case["samples"]) - golden[f"{key}/out"]).max(), bar + delta)


@pytest.mark.parametrize("name", list(mc.CONV_CASES))
def test_convolution_against_the_restatement_and_the_reference(conv_results, golden, name):
    case, want, got = conv_results[name]
    check(f"midas conv {name}", "conv/" + name, golden, case, got, want)


@pytest.mark.parametrize("name", list(mc.UPSAMPLE_CASES))
def test_upsampling_against_the_restatement_and_the_reference(upsample_results, golden, name):
    case, want, got = upsample_results[name]
    check(f"midas upsample2x {name}", "upsample/" + name, golden, case, got, want)
    if name.endswith("1x1"):
        assert got.shape == (1, 1, 2, 2) and (got == case["x"][0, 0, 0, 0]).all()


@pytest.mark.parametrize("name", list(mc.HEAD_CASES))
def test_head_against_the_restatement_and_the_reference(head_results, golden, name):
    case, want, got = head_results[name]
    check(f"midas head {name}", "head/" + name, golden, case, got, want)
    signed = mr.head(case["x"], case["weight2"], case["bias2"], case["weight4"], case["bias4"], False)
    assert (signed < 0).any() and (signed > 0).any()              # the last ReLU has work
    assert (got[signed < -1e-5] == 0).all() if case["non_negative"] else (got < 0).any()


@pytest.mark.parametrize("name", list(mc.DECODER_CASES))
def test_decoder_against_the_restatement_and_the_reference(decoder_results, golden, name):
    case, want, got = decoder_results[name]
    check(f"midas decoder {name}", "decoder/" + name, golden, case, got, want)


def test_the_in_place_relu_of_the_reference(solver, golden):
    """One ResidualConvUnit and one FeatureFusionBlock, chained through the operators, against the values the reference's own classes
    gave: their nn.ReLU(inplace=True) makes the skip relu(x).  The inputs' negative part is large; `+ x` would miss by more than 1."""
    case = mc.make_unit_case("rcu_64_6x7")
    got = unit(solver, case["x"], case["weights"], case["biases"])
    check("midas unit", "unit/rcu_64_6x7", golden, case, got, mr.unit_case(case))
    assert np.abs(got - mr.unit_case(case, inplace=False)).max() > 1.0
    case = mc.make_fusion_case("ffb_64_5x6b2")
    out = unit(solver, case["x1"], case["weights"][0:2], case["biases"][0:2], other=case["x0"])
    got = solver.midas_upsample2x(unit(solver, out, case["weights"][2:4], case["biases"][2:4]), align_corners=True)
    check("midas fusion block", "fusion/ffb_64_5x6b2", golden, case, got, mr.fusion_case(case))


def test_planted_is_exact(conv_results):
    """Small-integer weights, inputs and addends over S = 3 slices: exact in any order, so any miss is a whole number."""
    case, want, got = conv_results["planted_4x5b2"]
    assert api.midas_split(72 * 9, 20) == 3
    assert np.array_equal(got.astype(np.float64), want)


SPLIT_CASES = ("c2048_2x3", "c256_9x9b2", "c64_5x7b3", "k1_512_70_2x3", "c1024_4x6")


@pytest.mark.parametrize("name", SPLIT_CASES)
def test_split_k(solver, conv_results, golden, name):
    """The same case forced to S = 1 and at the rule's S > 1, both within the bar; and the split result is, bit for bit, the f64 sum
    in the order s = 0 .. S - 1 of its slices' own f32 partial sums, rounded once, with the epilogue in f32."""
    case, want, got = conv_results[name]
    Cin, k = case["x"].shape[1], case["k"]
    S = api.midas_split(Cin * k * k, case["x"].shape[2] * case["x"].shape[3], k)
    assert S > 1
    whole = run_conv(solver, case, split=1)
    check(f"midas conv {name} unsplit", "conv/" + name, golden, case, whole, want)
    assert np.array_equal(run_conv(solver, case, split=S), got)
    ranges = api.midas_slice_channels(Cin, k, S)
    assert len(ranges) == S
    total = np.zeros(got.shape, np.float64)
    for c0, c1 in ranges:
        total += solver.midas_conv(case["x"][:, c0:c1], case["weight"][:, c0:c1], None, relu_in=case["relu_in"], split=1)
    t = total.astype(np.float32)
    if case["bias"] is not None:
        t = t + case["bias"].reshape(1, -1, 1, 1)
    if case["relu"]:
        t = np.maximum(t, np.float32(0))
    if case["a"] is not None:
        t = t + (np.maximum(case["a"], np.float32(0)) if case["relu_a"] else case["a"])
    if case["b"] is not None:
        t = case["b"] + t
    assert t.dtype == np.float32 and np.array_equal(t, got)


def test_results_repeat_bit_for_bit(solver, conv_results, upsample_results, head_results, decoder_results):
    for name in ("c2048_1x1", "c256_9x9b2", "c21_19_5x7", "k1_512_70_2x3"):
        case, _want, got = conv_results[name]
        assert np.array_equal(run_conv(solver, case), got), name
    case, _want, got = upsample_results["aligned_12x20b2"]
    assert np.array_equal(solver.midas_upsample2x(case["x"], True), got)
    case, _want, got = head_results["5x7b2"]
    assert np.array_equal(run_head(solver, case), got)
    for name in ("f256_64x96", "f64_64x64"):
        case, _want, got = decoder_results[name]
        assert np.array_equal(run_decoder(solver, case), got), name


def test_a_batch_is_its_images_one_by_one(solver, conv_results, upsample_results, head_results, decoder_results):
    """B > 1 (tiles straddle rows and images; S > 1 for the convolution) against calls at B = 1: no pixel of a neighbouring image is
    read as halo, and the split does not depend on the batch."""
    for name in ("c64_5x7b3", "c256_9x9b2", "c21_19_5x7", "k1_40_24_5x7"):
        case, _want, got = conv_results[name]
        for i in range(case["x"].shape[0]):
            one = run_conv(solver, case, x=case["x"][i:i + 1], a=None if case["a"] is None else case["a"][i:i + 1],
                           b=None if case["b"] is None else case["b"][i:i + 1])
            assert np.array_equal(one[0], got[i]), (name, i)
    for name in ("aligned_12x20b2", "half_12x20b2"):
        case, _want, got = upsample_results[name]
        for i in range(2):
            assert np.array_equal(solver.midas_upsample2x(case["x"][i:i + 1], case["align_corners"])[0], got[i]), (name, i)
    case, _want, got = head_results["5x7b2_signed"]
    for i in range(2):
        assert np.array_equal(run_head(solver, case, x=case["x"][i:i + 1])[0], got[i]), i
    case, _want, got = decoder_results["f256_96x64b2"]
    for i in range(2):
        assert np.array_equal(run_decoder(solver, case, [m[i:i + 1] for m in case["maps"]])[0], got[i]), i


@pytest.mark.parametrize("name", ["f256_32x32", "f256_96x64b2", "f64_64x64"])
def test_the_decoder_is_its_stages_chained(solver, decoder_results, name):
    """midas_decoder against the same stages through midas_conv, midas_upsample2x and midas_head, bit for bit: scratch aliasing and
    layer-order mistakes apart from numerics.  The caller's feature maps are as they were."""
    case, _want, got = decoder_results[name]
    before = [m.copy() for m in case["maps"]]
    assert np.array_equal(chain(solver, case), got)
    assert all(np.array_equal(a, b) for a, b in zip(before, case["maps"]))


def _hip():
    return api._hip_runtime()


def test_refusals(solver):
    conv = mc.make_conv_case("c64_5x7b3")
    x, w, bias, a = conv["x"], conv["weight"], conv["bias"], conv["a"]
    head = mc.make_head_case("5x7b2")
    hx, w2, b2, w4, b4 = head["x"], head["weight2"], head["bias2"], head["weight4"], head["bias4"]
    dec = mc.make_decoder_case("f64_64x64")
    maps, ws, bs = dec["maps"], dec["weights"], dec["biases"]
    _hip().hipGetLastError()      # (the runtime keeps the last error of the thread until it is asked for)
    refused = [
        (TypeError, lambda: solver.midas_conv(x.astype(np.float64), w, bias)),
        (TypeError, lambda: solver.midas_conv(x, w, bias, a=a.astype(np.float16))),
        (ValueError, lambda: solver.midas_conv(x, np.zeros((64, 64, 5, 5), np.float32), bias)),
        (ValueError, lambda: solver.midas_conv(x, np.zeros((64, 64, 3, 1), np.float32), bias)),
        (ValueError, lambda: solver.midas_conv(x[:, :32], w, bias)),
        (ValueError, lambda: solver.midas_conv(x[:0], w, bias)),
        (ValueError, lambda: solver.midas_conv(x[0], w, bias)),
        (ValueError, lambda: solver.midas_conv(x, w, bias[:10])),
        (ValueError, lambda: solver.midas_conv(x, w, bias, a=a[:, :, :1])),
        (ValueError, lambda: solver.midas_conv(x, w, bias, b=a[:1])),
        (ValueError, lambda: solver.midas_conv(x, w, bias, split=9)),
        (ValueError, lambda: solver.midas_conv(x, w, bias, split=-1)),
        (TypeError, lambda: solver.midas_upsample2x(x.astype(np.float64))),
        (ValueError, lambda: solver.midas_upsample2x(x[0])),
        (ValueError, lambda: solver.midas_upsample2x(x[:, :, :0])),
        (TypeError, lambda: solver.midas_head(hx, w2.astype(np.float64), b2, w4, b4)),
        (ValueError, lambda: solver.midas_head(hx, w2[:16], b2[:16], w4[:, :16], b4)),        # a middle width other than 32
        (ValueError, lambda: solver.midas_head(hx[:, :64], w2, b2, w4, b4)),
        (ValueError, lambda: solver.midas_head(hx, w2, b2, w4, b4[:0])),
        (TypeError, lambda: solver.midas_decoder([m.astype(np.float64) for m in maps], ws, bs)),
        (ValueError, lambda: solver.midas_decoder(maps[:3], ws, bs)),
        (ValueError, lambda: solver.midas_decoder([maps[0], maps[1], maps[2], maps[3][:, :, :1]], ws, bs)),   # not an exact halving
        (ValueError, lambda: solver.midas_decoder([maps[0][:, :, :15], maps[1], maps[2], maps[3]], ws, bs)),
        (ValueError, lambda: solver.midas_decoder([maps[0][:0], maps[1], maps[2], maps[3]], ws, bs)),
        (ValueError, lambda: solver.midas_decoder(maps, ws[::-1], bs)),
        (ValueError, lambda: solver.midas_decoder(maps, ws[:20], bs)),
        (ValueError, lambda: solver.midas_decoder(maps, ws, bs[:16])),
        (ValueError, lambda: solver.midas_decoder([maps[0], maps[1][:, :100], maps[2], maps[3]], ws, bs)),
    ]
    for exc, call in refused:
        with pytest.raises(exc):
            call()
    assert _hip().hipDeviceSynchronize() == 0 and _hip().hipGetLastError() == 0
    # a null bias is fine
    assert np.isfinite(solver.midas_conv(x, w, None)).all()


def test_the_entry_points_refuse_too(solver):
    """The C ABI's own checks (a caller that bypasses the Python layer): an error that names the value, no launch, and the next good
    call works."""
    p = 1 << 24                # never dereferenced: every call below is rejected before any device work

    def conv(B=1, H=5, W=7, cin=64, cout=64, k=3, x=2 * p, w=3 * p, b=4 * p, relu_in=1, relu=0, a=5 * p, relu_a=1, b2=6 * p, split=0, out=7 * p):
        return solver._fn("midas_conv_device")(
            solver._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(cin), C.c_int32(cout), C.c_int32(k), C.c_void_p(x), C.c_void_p(w),
            C.c_void_p(b), C.c_int32(relu_in), C.c_int32(relu), C.c_void_p(a), C.c_int32(relu_a), C.c_void_p(b2), C.c_int32(split),
            C.c_void_p(out), None)

    def up(B=1, Cn=3, H=5, W=7, align=1, x=2 * p, out=3 * p):
        return solver._fn("midas_upsample2x_device")(solver._h, C.c_int32(B), C.c_int32(Cn), C.c_int32(H), C.c_int32(W), C.c_int32(align),
                                                     C.c_void_p(x), C.c_void_p(out), None)

    def head(B=1, H=5, W=7, cin=128, mid=32, x=2 * p, w2=3 * p, b2=4 * p, w4=5 * p, b4=6 * p, nn=1, out=7 * p):
        return solver._fn("midas_head_device")(
            solver._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(cin), C.c_int32(mid), C.c_void_p(x), C.c_void_p(w2),
            C.c_void_p(b2), C.c_void_p(w4), C.c_void_p(b4), C.c_int32(nn), C.c_void_p(out), None)

    four = (C.c_void_p * 4)(2 * p, 3 * p, 4 * p, 5 * p)
    w21 = (C.c_void_p * 21)(*([10 * p] * 21))
    b17 = (C.c_void_p * 17)(*([11 * p] * 17))

    def dec(B=1, features=64, channels=(256, 512, 1024, 2048), heights=(16, 8, 4, 2), widths=(24, 12, 6, 3), maps=four, weights=w21,
            biases=b17, nn=1, out=12 * p):
        return solver._fn("midas_decoder_device")(
            solver._h, C.c_int32(B), C.c_int32(features), (C.c_int32 * 4)(*channels), (C.c_int32 * 4)(*heights), (C.c_int32 * 4)(*widths),
            maps, weights, biases, C.c_int32(nn), C.c_void_p(out), None)

    _hip().hipGetLastError()
    cases = [(conv, dict(B=0), ">= 1"), (conv, dict(W=0), ">= 1"), (conv, dict(H=-3), ">= 1"),
             (conv, dict(k=5), "kernel_size must be 1 or 3 \\(got 5\\)"), (conv, dict(k=7), "kernel_size"), (conv, dict(k=2), "kernel_size"),
             (conv, dict(cin=0), "in_channels"), (conv, dict(cout=0), "out_channels"), (conv, dict(relu=2), "relu must be 0 or 1 \\(got 2\\)"),
             (conv, dict(relu_in=-1), "relu_in must be 0 or 1"), (conv, dict(relu_a=3), "relu_a must be 0 or 1"),
             (conv, dict(split=9), "split must be 0 \\(the rule\\) or 1 .. 8, the chunks of K \\(got 9\\)"), (conv, dict(split=-1), "split"),
             (conv, dict(x=None), "null"), (conv, dict(w=None), "null"), (conv, dict(out=None), "null"),
             (conv, dict(H=65536, W=65536), "exceed 2\\^31"),
             (conv, dict(out=2 * p + 64), "out overlaps x"), (conv, dict(out=5 * p + 128), "out overlaps the addend a"),
             (conv, dict(out=6 * p + 128), "out overlaps the addend b"),
             (up, dict(B=0), ">= 1"), (up, dict(Cn=0), ">= 1"), (up, dict(H=0), ">= 1"), (up, dict(align=2), "align_corners must be 0 or 1"),
             (up, dict(x=None), "null"), (up, dict(out=None), "null"), (up, dict(H=32768, W=32768), "exceed 2\\^31"),
             (up, dict(out=2 * p + 4), "out overlaps x"),
             (head, dict(B=0), ">= 1"), (head, dict(W=0), ">= 1"), (head, dict(cin=0), "in_channels"),
             (head, dict(mid=16), "mid_channels must be 32 \\(got 16\\)"), (head, dict(nn=2), "non_negative must be 0 or 1"),
             (head, dict(x=None), "null"), (head, dict(b2=None), "null"), (head, dict(w4=None), "null"), (head, dict(b4=None), "null"),
             (head, dict(out=None), "null"), (head, dict(H=65536, W=65536), "exceed 2\\^31"), (head, dict(out=2 * p + 8), "out overlaps x"),
             (dec, dict(B=0), ">= 1"), (dec, dict(features=0), "features must be >= 1 \\(got 0\\)"),
             (dec, dict(heights=(16, 8, 4, 0)), ">= 1"), (dec, dict(channels=(256, 0, 1024, 2048)), "channels of feature map 2"),
             (dec, dict(heights=(16, 8, 4, 3)), "feature map 3 is 4 x 6, not twice map 4's 3 x 3"),
             (dec, dict(widths=(25, 12, 6, 3)), "feature map 1 is 16 x 25, not twice map 2's 8 x 12"),
             (dec, dict(heights=(1 << 17, 1 << 16, 1 << 15, 1 << 14), widths=(1 << 17, 1 << 16, 1 << 15, 1 << 14)), "exceed 2\\^31"),
             (dec, dict(heights=(1 << 15, 1 << 14, 1 << 13, 1 << 12), widths=(1 << 15, 1 << 14, 1 << 13, 1 << 12)), "exceed 2\\^31"),
             (dec, dict(maps=None), "null"), (dec, dict(weights=None), "null"), (dec, dict(biases=None), "null"), (dec, dict(out=None), "null"),
             (dec, dict(maps=(C.c_void_p * 4)(2 * p, None, 4 * p, 5 * p)), "null feature map 2"),
             (dec, dict(weights=(C.c_void_p * 21)(*([10 * p] * 7 + [None] + [10 * p] * 13))), "null weight 7"),
             (dec, dict(biases=(C.c_void_p * 17)(*([11 * p] * 16 + [None]))), "null bias 16"),
             (dec, dict(nn=-1), "non_negative"), (dec, dict(out=3 * p + 16), "out overlaps feature map 2")]
    for fn, kwargs, word in cases:
        with pytest.raises(RuntimeError, match=word):
            solver._check(fn(**kwargs))
    assert _hip().hipDeviceSynchronize() == 0 and _hip().hipGetLastError() == 0
    case = mc.make_conv_case("c64_8x8")
    assert np.isfinite(run_conv(solver, case)).all()


def test_torch_modules():
    """robust_cvd_amd.midas on GPU tensors, in a fresh process: torch has to be imported before libcvd_hip.so is loaded.  The checks
    are tests/midas_torch_child.py's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.midas_torch_child"], cwd=root, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "midas torch modules ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
