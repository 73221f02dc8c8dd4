"""GPU checks of the encoder kernels (robust_cvd_amd/csrc/cvd_raftenc.h) through the array paths
(Solver.raft_encoder_conv, Solver.raft_instance_norm, Solver.raft_encoder) and, in a fresh process, through the torch drop-ins
robust_cvd_amd.raft_ops.BasicEncoder and RAFT (tests/raftenc_torch_child.py).

Bar: |kernel - f64| <= 8 x max(delta, 2^-23 x scale) against the float64 restatement (tests/raftenc_reference.py), delta = the
REFERENCE's own f32 error against that restatement for the case, scale = the largest |output|, both read from the fixture
(tests/golden/reference_py/raftenc_golden.npz, minted on the CPU; never from these kernels); against the reference's stored f32
values that bar + delta.  The factor 8 is the one the project's other f32 kernels carry (tests/test_gpu_raftblock.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import margins
from tests import raftenc_cases as ec
from tests import raftenc_reference as er

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from robust_cvd_amd.api import Solver
    return Solver(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(er.GOLDEN)


def run_conv(solver, case, **over):
    c = dict(case, **over)
    return solver.raft_encoder_conv(c["x"], c["weight"], c["bias"], stride=c["stride"], norm=c["norm"], eps=ec.EPS, relu=c["relu"],
                                    residual=c["residual"])


def run_norm(solver, case, inplace=False, **over):
    c = dict(case, **over)
    return solver.raft_instance_norm(c["x"], eps=ec.EPS, relu=c["relu"], residual=c["residual"], inplace=inplace)


def run_encoder(solver, case, images=None):
    return solver.raft_encoder(case["images"] if images is None else images, case["weights"], case["biases"], norm=case["norm_mode"],
                               norms=case["norms"] if case["norm_mode"] == "batch" else None, eps=ec.EPS)


def chain(solver, case):
    """The encoder's stages one by one through raft_encoder_conv and raft_instance_norm, as cvd_raft_encoder_device chains them."""
    mode, w, b = case["norm_mode"], case["weights"], case["biases"]

    def layer(i, x, relu, residual=None):
        stride = ec.LAYERS[i][4]
        if mode == "instance" and i < 15:
            y = solver.raft_encoder_conv(x, w[i], b[i], stride=stride)
            return solver.raft_instance_norm(y, eps=ec.EPS, relu=relu, residual=residual, inplace=True)
        return solver.raft_encoder_conv(x, w[i], b[i], stride=stride, norm=case["norms"][i] if mode == "batch" and i < 15 else None,
                                        eps=ec.EPS, relu=relu, residual=residual)

    def block(i, x, strided):
        y = layer(i, x, True)
        if strided:
            x = layer(i + 2, x, False)
        return layer(i + 1, y, True, x)
    x = layer(0, case["images"], True)
    x = block(3, block(1, x, False), False)
    x = block(8, block(5, x, True), False)
    x = block(13, block(10, x, True), False)
    return layer(15, x, False)


@pytest.fixture(scope="module")
def conv_results(solver):
    """Per single-convolution case: (inputs, f64 restatement, kernel output): computed once, shared."""
    out = {}
    for name in ec.CONV_CASES:
        case = ec.make_conv_case(name)
        out[name] = (case, er.conv_case(case), run_conv(solver, case))
    return out


@pytest.fixture(scope="module")
def norm_results(solver):
    out = {}
    for name in ec.NORM_CASES:
        case = ec.make_norm_case(name)
        out[name] = (case, er.norm_case(case), run_norm(solver, case))
    return out


@pytest.fixture(scope="module")
def encoder_results(solver):
    out = {}
    for name in ec.ENCODER_CASES:
        case = ec.make_encoder_case(name)
        out[name] = (case, er.encoder_case(case), run_encoder(solver, case))
    return out


def check(label, key, golden, case, got, want):
    assert ec.input_digest(case) == golden[f"{key}/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    delta = float(golden[f"{key}/out_delta"])
    bar = er.bar(delta, golden[f"{key}/out_scale"])
    err = np.abs(got - want).max()
    print(f"{key}: max |kernel - f64| {err:.3e}, bar {bar:.3e}, share {err / bar if bar else 0.0:.3f} (reference's own delta {delta:.3e})")
    if bar == 0.0:          # an output of zeros (one pixel under a ReLU): exact
        assert err == 0.0
        return
    margins.below(label, err, bar)
    margins.below(f"{label} vs reference", np.abs(ec.sample_view(got, case["samples"]) - golden[f"{key}/out"]).max(), bar + delta)


@pytest.mark.parametrize("name", list(ec.CONV_CASES))
def test_convolution_against_the_restatement_and_the_reference(conv_results, golden, name):
    case, want, got = conv_results[name]
    check(f"raft encoder conv {name}", "conv/" + name, golden, case, got, want)


@pytest.mark.parametrize("name", list(ec.NORM_CASES))
def test_instance_norm_against_the_restatement_and_the_reference(norm_results, golden, name):
    case, want, got = norm_results[name]
    check(f"raft instance norm {name}", "norm/" + name, golden, case, got, want)


@pytest.mark.parametrize("name", list(ec.ENCODER_CASES))
def test_encoder_against_the_restatement_and_the_reference(encoder_results, golden, name):
    case, want, got = encoder_results[name]
    check(f"raft encoder {name}", "encoder/" + name, golden, case, got, want)


def test_results_repeat_bit_for_bit(solver, conv_results, norm_results, encoder_results):
    for name in ("c7s2_3x5x7", "c3s2_128_2x6x8", "c3_128_1x2x130", "c1_256_3x5x7"):
        case, _want, got = conv_results[name]
        assert np.array_equal(run_conv(solver, case), got), name
    for name in ("in_9100", "in_35"):
        case, _want, got = norm_results[name]
        assert np.array_equal(run_norm(solver, case), got), name
    for name in ("instance_16x24b3", "batch_40x56"):
        case, _want, got = encoder_results[name]
        assert np.array_equal(run_encoder(solver, case), got), name


def test_a_batch_is_its_images_one_by_one(solver, conv_results, norm_results, encoder_results):
    """B = 3 (a tile of 64 output pixels straddles rows and images) against calls at B = 1: no pixel of a neighbouring image is read
    as halo, no plane's statistics leak."""
    for kind in ec.CONV_KINDS:
        name = f"{kind}_3x5x7"
        case, _want, got = conv_results[name]
        for i in range(3):
            one = run_conv(solver, case, x=case["x"][i:i + 1], residual=None if case["residual"] is None else case["residual"][i:i + 1])
            assert np.array_equal(one[0], got[i]), (name, i)
    case, _want, got = norm_results["in_35"]
    for i in range(2):
        assert np.array_equal(run_norm(solver, case, x=case["x"][i:i + 1], residual=case["residual"][i:i + 1])[0], got[i]), i
    for name in ("none_16x24b3", "instance_16x24b3", "batch_16x24b3", "instance_13x9b2"):
        case, _want, got = encoder_results[name]
        for i in range(case["images"].shape[0]):
            assert np.array_equal(run_encoder(solver, case, case["images"][i:i + 1])[0], got[i]), (name, i)


@pytest.mark.parametrize("name", ["none_16x24b3", "instance_16x24b3", "batch_16x24b3", "instance_9x9", "batch_40x56"])
def test_the_encoder_is_its_stages_chained(solver, encoder_results, name):
    """raft_encoder against the same stages through raft_encoder_conv and raft_instance_norm, bit for bit: scratch aliasing and
    layer-order mistakes apart from numerics."""
    case, _want, got = encoder_results[name]
    assert np.array_equal(chain(solver, case), got)


def test_in_place_instance_norm_is_out_of_place(solver, norm_results):
    for name, (case, _want, got) in norm_results.items():
        assert np.array_equal(run_norm(solver, case, inplace=True), got), name


def test_planted_is_exact(conv_results, norm_results, encoder_results):
    _case, _want, got = conv_results["planted_3x5x7"]
    for ch, value in ec.PLANTED[0].items():
        assert (got[:, ch] == max(np.float32(value), np.float32(0.0))).all(), ch
    for ch in ec.PLANTED[1]:
        assert (got[:, ch] == 0.0).all(), ch
    _case, _want, got = encoder_results["planted"]
    for ch, value in ec.PLANTED_ENCODER.items():
        assert (got[:, ch] == np.float32(value)).all(), ch
    _case, _want, got = norm_results["in_const"]
    assert (got[:, 0] == 0.0).all()


def _hip():
    from robust_cvd_amd import api
    return api._hip_runtime()


def test_refusals(solver):
    conv = ec.make_conv_case("c3_64_1x2x3")
    x, w, b, norm, res = conv["x"], conv["weight"], conv["bias"], conv["norm"], conv["residual"]
    enc = ec.make_encoder_case("batch_9x9")
    im, ws, bs, ns = enc["images"], enc["weights"], enc["biases"], enc["norms"]
    _hip().hipGetLastError()      # (the runtime keeps the last error of the thread until it is asked for)
    refused = [
        (TypeError, lambda: solver.raft_encoder_conv(x.astype(np.float64), w, b)),
        (TypeError, lambda: solver.raft_encoder_conv(x, w, b, norm=[v.astype(np.float64) for v in norm])),
        (ValueError, lambda: solver.raft_encoder_conv(x, w, b, stride=3)),
        (ValueError, lambda: solver.raft_encoder_conv(x, np.zeros((64, 64, 5, 5), np.float32), b)),
        (ValueError, lambda: solver.raft_encoder_conv(x[:, :32], w, b)),
        (ValueError, lambda: solver.raft_encoder_conv(x[:0], w, b)),
        (ValueError, lambda: solver.raft_encoder_conv(x, w, b[:10])),
        (ValueError, lambda: solver.raft_encoder_conv(x, w, b, norm=norm[:3])),
        (ValueError, lambda: solver.raft_encoder_conv(x, w, b, norm=norm, eps=0.0)),
        (ValueError, lambda: solver.raft_encoder_conv(x, w, b, residual=res[:, :, :1])),
        (TypeError, lambda: solver.raft_instance_norm(x.astype(np.float16))),
        (ValueError, lambda: solver.raft_instance_norm(x[:, :, :1, :1])),
        (ValueError, lambda: solver.raft_instance_norm(x, eps=-1.0)),
        (ValueError, lambda: solver.raft_instance_norm(x, residual=x[:, :1])),
        (ValueError, lambda: solver.raft_instance_norm(x[0])),
        (TypeError, lambda: solver.raft_encoder(im.astype(np.float64), ws, bs)),
        (ValueError, lambda: solver.raft_encoder(im, ws, bs, norm="group")),
        (ValueError, lambda: solver.raft_encoder(im, ws, bs, norm="batch")),
        (ValueError, lambda: solver.raft_encoder(im, ws, bs, norm="batch", norms=ns[:14])),
        (ValueError, lambda: solver.raft_encoder(im, ws, bs, norm="batch", norms=ns, eps=0.0)),
        (ValueError, lambda: solver.raft_encoder(im[:, :2], ws, bs)),
        (ValueError, lambda: solver.raft_encoder(im, ws[::-1], bs)),
        (ValueError, lambda: solver.raft_encoder(im, ws[:15], bs[:15])),
        (ValueError, lambda: solver.raft_encoder(im[:, :, :8, :8], ws, bs, norm="instance")),
    ]
    for exc, call in refused:
        with pytest.raises(exc):
            call()
    assert _hip().hipDeviceSynchronize() == 0 and _hip().hipGetLastError() == 0
    # 8 x 8 images give one feature pixel: fine without instance norm
    assert solver.raft_encoder(im[:, :, :8, :8], ws, bs).shape == (1, 256, 1, 1)


def test_the_entry_points_refuse_too(solver):
    """The C ABI's own checks (a caller that bypasses the Python layer): an error that names the value, no launch, and the next
    good call works."""
    p = 1 << 24                # never dereferenced: every call below is rejected before any device work
    four = (C.c_void_p * 4)(*([9 * p] * 4))

    def conv(B=1, H=5, W=7, cin=64, cout=64, k=3, stride=1, x=2 * p, w=3 * p, b=4 * p, norm=four, eps=1e-5, relu=1, res=5 * p, out=6 * p):
        return solver._fn("raft_encoder_conv_device")(
            solver._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(cin), C.c_int32(cout), C.c_int32(k), C.c_int32(stride),
            C.c_void_p(x), C.c_void_p(w), C.c_void_p(b), norm, C.c_float(eps), C.c_int32(relu), C.c_void_p(res), C.c_void_p(out), None)

    def norm(B=1, Cn=64, H=5, W=7, x=2 * p, eps=1e-5, relu=1, res=3 * p, out=4 * p):
        return solver._fn("raft_instance_norm_device")(
            solver._h, C.c_int32(B), C.c_int32(Cn), C.c_int32(H), C.c_int32(W), C.c_void_p(x), C.c_float(eps), C.c_int32(relu),
            C.c_void_p(res), C.c_void_p(out), None)

    sixteen = (C.c_void_p * 16)(*([10 * p] * 16))
    sixty = (C.c_void_p * 60)(*([11 * p] * 60))

    def enc(B=1, H=16, W=24, dim=256, mode=2, eps=1e-5, images=2 * p, weights=sixteen, biases=sixteen, norms=sixty, out=3 * p):
        return solver._fn("raft_encoder_device")(
            solver._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(dim), C.c_int32(mode), C.c_float(eps), C.c_void_p(images),
            weights, biases, norms, C.c_void_p(out), None)

    _hip().hipGetLastError()
    cases = [(conv, dict(B=0), ">= 1"), (conv, dict(W=0), ">= 1"), (conv, dict(H=-3), ">= 1"),
             (conv, dict(k=5), "kernel_size must be 1, 3 or 7 \\(got 5\\)"), (conv, dict(k=2), "kernel_size"),
             (conv, dict(stride=3), "stride must be 1 or 2 \\(got 3\\)"), (conv, dict(stride=0), "stride"),
             (conv, dict(cin=0), "in_channels"), (conv, dict(cout=0), "out_channels"), (conv, dict(relu=2), "relu must be 0 or 1"),
             (conv, dict(x=None), "null"), (conv, dict(w=None), "null"), (conv, dict(b=None), "null"), (conv, dict(out=None), "null"),
             (conv, dict(norm=(C.c_void_p * 4)(9 * p, None, 9 * p, 9 * p)), "null norm vector 1"),
             (conv, dict(eps=0.0), "eps must be > 0"), (conv, dict(eps=-1e-5), "eps"),
             (conv, dict(H=65536, W=65536), "exceed 2\\^31"),
             (conv, dict(out=2 * p + 64), "out overlaps x"), (conv, dict(out=5 * p + 128), "out overlaps the residual"),
             (norm, dict(B=0), ">= 1"), (norm, dict(Cn=0), ">= 1"), (norm, dict(H=1, W=1), "planes of 1 element"),
             (norm, dict(eps=0.0), "eps must be > 0"), (norm, dict(x=None), "null"), (norm, dict(out=None), "null"),
             (norm, dict(relu=-1), "relu"), (norm, dict(H=65536, W=32768), "exceed 2\\^31"),
             (norm, dict(out=2 * p + 4), "out overlaps x"), (norm, dict(out=3 * p + 4), "out overlaps the residual"),
             (enc, dict(B=0), ">= 1"), (enc, dict(H=0), ">= 1"), (enc, dict(dim=0), "output_dim"),
             (enc, dict(mode=3), "norm_mode must be 0 \\(none\\), 1 \\(instance\\) or 2 \\(batch\\) \\(got 3\\)"), (enc, dict(mode=-1), "norm_mode"),
             (enc, dict(eps=0.0), "eps must be > 0"), (enc, dict(images=None), "null"), (enc, dict(out=None), "null"),
             (enc, dict(norms=None), "null"), (enc, dict(weights=None), "null"),
             (enc, dict(weights=(C.c_void_p * 16)(*([10 * p] * 7 + [None] + [10 * p] * 8))), "null weight or bias 7"),
             (enc, dict(norms=(C.c_void_p * 60)(*([11 * p] * 59 + [None]))), "null norm vector 59"),
             (enc, dict(mode=1, H=8, W=8), "planes of 1 element"), (enc, dict(H=65536, W=65536), "exceed 2\\^31"),
             (enc, dict(out=2 * p + 16), "out overlaps the images")]
    for fn, kwargs, word in cases:
        with pytest.raises(RuntimeError, match=word):
            solver._check(fn(**kwargs))
    assert _hip().hipDeviceSynchronize() == 0 and _hip().hipGetLastError() == 0
    case = ec.make_encoder_case("instance_9x9")
    assert np.isfinite(run_encoder(solver, case)).all()


def test_torch_modules():
    """robust_cvd_amd.raft_ops.BasicEncoder and RAFT on GPU tensors, in a fresh process: torch has to be imported before
    libcvd_hip.so is loaded.  The checks are tests/raftenc_torch_child.py's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.raftenc_torch_child"], cwd=root, capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "raft encoder torch modules ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
