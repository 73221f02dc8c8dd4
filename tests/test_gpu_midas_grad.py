"""GPU checks of the backward kernels of the MiDaS decoder's layers (robust_cvd_amd/csrc/cvd_midas_grad.h) through
the array paths Solver.midas_conv_grad_input, midas_conv_grad_weight, midas_upsample2x_grad, midas_head_grad, midas_decoder_train and
midas_decoder_backward (at features 256 checked bit for bit against the inference decoder and the chained operators: not against f64,
because of ReLU ties) and, in a fresh
process, through the torch layer robust_cvd_amd.midas_train (tests/midas_grad_torch_child.py).

Bar, per gradient tensor: |kernel - f64| <= 8 x max(delta, 2^-23 x scale) against the float64 restatement
(tests/midas_grad_reference.py), delta = torch autograd's own f32 error against that restatement for the case, scale = the largest
|gradient|, both read from the fixture (tests/golden/reference_py/midas_grad_golden.npz, minted on the CPU; never from these kernels);
against the stored f32 samples that bar + delta.  The masks of the convolution cases are given f32 tensors, so no ReLU tie can flip
them; the head cases' masks are computed, and tests/test_midas_grad_reference.py holds their tie condition.

The planted case 72 -> 40 at 2 x 4 x 5 runs with a forced split of 3, which the operators shrink to whole chains (two chains of K for
the input gradient; 40 pixels are one chain of the weight gradient); planted_12x16b2 is the same layer over 384 pixels, where the
forced split does cut the weight gradient's pixels in two."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from robust_cvd_amd import api
from tests import margins
from tests import midas_grad_cases as gc
from tests import midas_grad_reference as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    return api.Solver(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(gr.GOLDEN)


def run_conv_grads(solver, case, split=None):
    split = case["split"] if split is None else split
    gx = solver.midas_conv_grad_input(case["gy"], case["weight"], add=case["add"], mask=case["mask"],
                                      split=min(split, -(-case["gy"].shape[1] // (32 if case["k"] == 1 else 8))))
    gw, gb = solver.midas_conv_grad_weight(case["gy"], case["x"], case["k"], relu_in=case["relu_in"], split=split)
    return {"gx": gx, "gw": gw, "gb": gb}


@pytest.fixture(scope="module")
def conv_results(solver):
    """Per case: (inputs, f64 restatement, kernel outputs): computed once, shared."""
    out = {}
    for name in gc.CONV_GRAD_CASES:
        case = gc.make_conv_grad_case(name)
        before = {k: v.copy() for k, v in case.items() if isinstance(v, np.ndarray)}
        out[name] = (case, gr.conv_grad_case(case), run_conv_grads(solver, case))
        assert all((case[k] == v).all() for k, v in before.items()), "an input was modified"
    return out


@pytest.fixture(scope="module")
def upsample_results(solver):
    out = {}
    for name in gc.UPSAMPLE_GRAD_CASES:
        case = gc.make_upsample_grad_case(name)
        out[name] = (case, gr.upsample_grad_case(case), {"gx": solver.midas_upsample2x_grad(case["gy"], case["align_corners"])})
    return out


def check(label, key, golden, case, got, want):
    assert gc.input_digest(case) == golden[f"{key}/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    for tensor in want:
        g, w = got[tensor], want[tensor]
        assert g.shape == w.shape and g.dtype == np.float32 and np.isfinite(g).all(), (key, tensor)
        delta = float(golden[f"{key}/{tensor}_delta"])
        bar = gr.bar(delta, golden[f"{key}/{tensor}_scale"])
        err = np.abs(g - w).max()
        print(f"{key}/{tensor}: max |kernel - f64| {err:.3e}, bar {bar:.3e}, share {err / bar if bar else 0.0:.3f} (torch's own delta {delta:.3e})")
        margins.below(f"{label} {tensor}", err, bar)
        margins.below(f"{label} {tensor} vs reference", np.abs(g.reshape(-1)[case["samples"][tensor]] - golden[f"{key}/{tensor}"]).max(),
                      bar + delta)


@pytest.mark.parametrize("name", list(gc.CONV_GRAD_CASES))
def test_convolution_gradients_against_the_restatement_and_the_reference(conv_results, golden, name):
    case, want, got = conv_results[name]
    check(f"midas conv grad {name}", "conv/" + name, golden, case, got, want)
    if case["mask"] is not None:
        assert (got["gx"][case["mask"] <= 0] == 0).all() and (got["gx"][case["mask"] > 0] != 0).any()
    if name.startswith("planted"):
        for tensor in want:
            assert (got[tensor] == want[tensor]).all(), f"{tensor}: exact integers"


def test_a_single_pixel_reaches_the_centre_tap_alone(conv_results):
    case, _want, got = conv_results["g2048_1x1"]
    off = np.ones((3, 3), bool)
    off[1, 1] = False
    assert (got["gw"][:, :, off] == 0).all() and (got["gw"][:, :, 1, 1] != 0).any()
    assert (got["gb"] == case["gy"][0, :, 0, 0]).all()


def test_weight_gradient_split_by_the_rule_and_unsplit(solver, conv_results, golden):
    """64 -> 64 at 3 x 24 x 40: S = 12 by the rule; forced to one slice: both within the bar, and their difference within it."""
    name = "g64_24x40b3"
    case, want, got = conv_results[name]
    B, N, H, W = case["gy"].shape
    assert api.midas_wgrad_split(B * H * W, N, case["x"].shape[1] * 9) == 12
    gw1, gb1 = solver.midas_conv_grad_weight(case["gy"], case["x"], 3, relu_in=case["relu_in"], split=1)
    bar = gr.bar(golden[f"conv/{name}/gw_delta"], golden[f"conv/{name}/gw_scale"])
    margins.below("midas wgrad forced split 1", np.abs(gw1 - want["gw"]).max(), bar)
    margins.below("midas wgrad split 12 - split 1", np.abs(gw1 - got["gw"]).max(), bar)
    assert (gb1 == got["gb"]).all()
    # the planted case over 384 pixels: the forced split cuts the pixels in two, the unsplit run does not; both exact
    case, want, got = conv_results["planted_12x16b2"]
    gw1, _ = solver.midas_conv_grad_weight(case["gy"], case["x"], 3, relu_in=True, split=1)
    assert (gw1 == want["gw"]).all() and (got["gw"] == want["gw"]).all()


def test_input_gradient_split_and_unsplit_and_by_image(solver, conv_results, golden):
    """2048 -> 256 at 2 x 3: K = 256 x 9 splits (S = 8 by the forward's rule); forced to 1: within the bar of each other.  A batch's
    input gradients are the bits of its images one by one."""
    name = "g2048_2x3"
    case, want, got = conv_results[name]
    assert api.midas_split(256 * 9, 6) == 8
    one = solver.midas_conv_grad_input(case["gy"], case["weight"], split=1)
    bar = gr.bar(golden[f"conv/{name}/gx_delta"], golden[f"conv/{name}/gx_scale"])
    margins.below("midas dgrad forced split 1", np.abs(one - want["gx"]).max(), bar)
    margins.below("midas dgrad split 8 - split 1", np.abs(one - got["gx"]).max(), bar)
    for name in ("g256_9x9b2", "g21_19_5x7b2"):
        case, _want, got = conv_results[name]
        for b in range(case["gy"].shape[0]):
            alone = solver.midas_conv_grad_input(case["gy"][b:b + 1], case["weight"], add=None if case["add"] is None else case["add"][b:b + 1],
                                                 mask=case["mask"][b:b + 1])
            assert (alone == got["gx"][b:b + 1]).all(), (name, b)


def test_the_gradients_repeat_bit_for_bit(solver, conv_results):
    for name in ("g64_24x40b3", "g21_19_5x7b2"):
        case, _want, got = conv_results[name]
        again = run_conv_grads(solver, case)
        assert all((again[k] == got[k]).all() for k in got), name


def test_the_bias_gradient_is_optional(solver, conv_results):
    case, _want, got = conv_results["g20_5x7"]
    gw, gb = solver.midas_conv_grad_weight(case["gy"], case["x"], 3, relu_in=True, bias=False)
    assert gb is None and (gw == got["gw"]).all()


@pytest.mark.parametrize("name", list(gc.UPSAMPLE_GRAD_CASES))
def test_upsampling_gradient_against_the_restatement_and_the_reference(upsample_results, golden, name):
    case, want, got = upsample_results[name]
    check(f"midas upsample2x grad {name}", "upsample/" + name, golden, case, got, want)
    if name.endswith("1x1"):
        four = case["gy"][0, 0].astype(np.float64).sum()
        assert got["gx"].shape == (1, 1, 1, 1) and abs(float(got["gx"][0, 0, 0, 0]) - four) <= 4 * gr.EPS32 * np.abs(case["gy"]).sum()


HEAD_KEYS = ("gx", "gw2", "gb2", "gw4", "gb4")


@pytest.fixture(scope="module")
def head_results(solver):
    out = {}
    for name in gc.HEAD_GRAD_CASES:
        case = gc.make_head_grad_case(name)
        got = solver.midas_head_grad(case["gy"], case["x"], case["weight2"], case["bias2"], case["weight4"], case["bias4"],
                                     non_negative=case["non_negative"])
        out[name] = (case, gr.head_grad_case(case), dict(zip(HEAD_KEYS, got)))
    return out


@pytest.mark.parametrize("name", list(gc.HEAD_GRAD_CASES))
def test_head_gradients_against_the_restatement_and_the_reference(solver, head_results, golden, name):
    case, want, got = head_results[name]
    check(f"midas head grad {name}", "head/" + name, golden, case, got, want)
    t, s = gr.head_forward(case)
    assert (t <= 0).any() and (s <= 0).any()                       # both masks have work
    y = solver.midas_head(case["x"], case["weight2"], case["bias2"], case["weight4"], case["bias4"], non_negative=case["non_negative"])
    assert ((y <= 0) == (s <= 0)).all() if case["non_negative"] else (y < 0).any()
    again = solver.midas_head_grad(case["gy"], case["x"], case["weight2"], case["bias2"], case["weight4"], case["bias4"],
                                   non_negative=case["non_negative"])
    assert all((a == got[k]).all() for k, a in zip(HEAD_KEYS, again)), "the head's gradients do not repeat bit for bit"


def test_the_recomputed_pre_activation_is_the_heads(solver, head_results):
    """The head's backward recomputes t with the plain convolution kernel at one slice.  With output_conv.4 a one-hot of channel n
    and no bias the head returns relu(t_n) itself (every other term is fmaf(v, 0, s) = s): it equals the recomputed tensor bit for
    bit, so the masks come from the forward's own f32 values."""
    case = head_results["5x7b2_signed"][0]
    t = solver.midas_conv(case["x"], case["weight2"], case["bias2"], split=1)
    for n in (0, 5, 18, 31):
        hot = np.zeros((1, 32, 1, 1), np.float32)
        hot[0, n] = 1.0
        y = solver.midas_head(case["x"], case["weight2"], case["bias2"], hot, np.zeros(1, np.float32), non_negative=False)
        assert (y == np.maximum(t[:, n], 0.0)).all(), n


# ---- the whole decoder: one call forward (train), one call backward ------------------------------------------------------------------
DECODER_BITS = ("f256_64x96", "f256_96x64b2")


def chained_backward(solver, case, saved, gy, map_gradients=True):
    """The decoder's backward through the four operator array paths, in cvd_midas_decoder_backward_device's order."""
    W, Bs, maps, nn = case["weights"], case["biases"], case["maps"], case["non_negative"]
    gw, gb, gm = [None] * 21, [None] * 17, [None] * 4

    def wgrad(idx, g, x, relu_in):
        gw[idx], bias = solver.midas_conv_grad_weight(g, x, 3, relu_in=relu_in, bias=idx >= 4)
        if idx >= 4:
            gb[idx - 4] = bias
    hup = solver.midas_upsample2x(saved[15], align_corners=False)
    ghup, gw[19], gb[15], gw[20], gb[16] = solver.midas_head_grad(gy, hup, W[19], Bs[15], W[20], Bs[16], non_negative=nn)
    gh0 = solver.midas_upsample2x_grad(ghup, align_corners=False)
    wgrad(18, gh0, saved[14], False)
    gp = solver.midas_conv_grad_input(gh0, W[18])
    for k in range(4):
        w0 = 4 if k == 3 else 6 + 4 * (2 - k)
        u2 = w0 if k == 3 else w0 + 2
        at = 5 + 3 * (2 - k)
        o, t2 = (saved[3], saved[4]) if k == 3 else (saved[at + 1], saved[at + 2])
        g = solver.midas_upsample2x_grad(gp, align_corners=True)
        wgrad(u2 + 1, g, t2, True)
        g1 = solver.midas_conv_grad_input(g, W[u2 + 1], mask=t2)
        wgrad(u2, g1, o, True)
        go = solver.midas_conv_grad_input(g1, W[u2], add=g, mask=o)
        gl = go
        if k < 3:
            wgrad(w0 + 1, go, saved[at], True)
            g1 = solver.midas_conv_grad_input(go, W[w0 + 1], mask=saved[at])
            wgrad(w0, g1, saved[k], True)
            gl = solver.midas_conv_grad_input(g1, W[w0], add=go, mask=saved[k])
        wgrad(k, gl, maps[k], False)
        if map_gradients:
            gm[k] = solver.midas_conv_grad_input(gl, W[k])
        gp = go
    return gw, gb, gm


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def decoder_runs(solver):
    """Per features-256 case: (case, gy, train output, saved table, one-call backward)."""
    from tests import midas_cases as mc
    out = {}
    for name in DECODER_BITS:
        case = mc.make_decoder_case(name)
        B, _, H, W = case["images"].shape
        gy = np.random.default_rng(len(name)).normal(0.0, 1.0, (B, H, W)).astype(np.float32)
        kept = [a.copy() for a in case["maps"] + case["weights"] + case["biases"]]
        y, saved = solver.midas_decoder_train(case["maps"], case["weights"], case["biases"], non_negative=case["non_negative"])
        grads = solver.midas_decoder_backward(gy, case["maps"], saved, case["weights"], case["biases"], non_negative=case["non_negative"])
        assert same(kept, case["maps"] + case["weights"] + case["biases"]), "the caller's inputs were modified"
        out[name] = (case, gy, y, saved, grads)
    return out


@pytest.mark.parametrize("name", DECODER_BITS)
def test_decoder_train_output_is_the_inference_decoders(solver, decoder_runs, name):
    case, _gy, y, saved, _grads = decoder_runs[name]
    assert (y == solver.midas_decoder(case["maps"], case["weights"], case["biases"], non_negative=case["non_negative"])).all()
    B, features = case["maps"][0].shape[0], case["features"]
    assert [a.shape for a in saved] == api.midas_saved_shapes(B, features, [m.shape[2] for m in case["maps"]], [m.shape[3] for m in case["maps"]])
    assert all(np.isfinite(a).all() and (a != 0).any() for a in saved)


@pytest.mark.parametrize("name", DECODER_BITS)
def test_decoder_backward_is_the_chained_operators_and_repeats(solver, decoder_runs, name):
    case, gy, _y, saved, (gw, gb, gm) = decoder_runs[name]
    cw, cb, cm = chained_backward(solver, case, saved, gy)
    assert same(gw, cw) and same(gb, cb) and same(gm, cm), "one call differs from the stages chained through the operator entry points"
    assert all(np.isfinite(a).all() and (a != 0).any() for a in gw + gb + gm)
    again = solver.midas_decoder_backward(gy, case["maps"], saved, case["weights"], case["biases"], non_negative=case["non_negative"])
    assert same(gw, again[0]) and same(gb, again[1]) and same(gm, again[2]), "two calls differ"
    # null map-gradient pointers: the parameter gradients are unchanged
    w2, b2, none = solver.midas_decoder_backward(gy, case["maps"], saved, case["weights"], case["biases"], non_negative=case["non_negative"],
                                                 map_gradients=False)
    assert none is None and same(gw, w2) and same(gb, b2)


@pytest.mark.parametrize("name", list(gc.SMALL_DECODER_CASES))
def test_small_decoder_gradients_against_the_restatement_and_the_reference(solver, golden, name):
    """Features 16 over the small stub (channels 16 / 21 / 40 / 72): all 38 parameter gradients and the four map gradients of the one-call
    backward against the f64 restatement and the reference's own MidasNet under autograd.  Seeds chosen for the tie condition."""
    case = gc.make_small_decoder_case(name)
    y, saved = solver.midas_decoder_train(case["maps"], case["weights"], case["biases"], non_negative=case["non_negative"])
    assert (y == solver.midas_decoder(case["maps"], case["weights"], case["biases"], non_negative=case["non_negative"])).all()
    gw, gb, gm = solver.midas_decoder_backward(case["gy"], case["maps"], saved, case["weights"], case["biases"], non_negative=case["non_negative"])
    got = {f"gw{i:02d}": a for i, a in enumerate(gw)}
    got.update({f"gb{i:02d}": a for i, a in enumerate(gb)})
    got.update({f"gm{k}": a for k, a in enumerate(gm)})
    want = gr.decoder_grad_case(case)
    want = {k: v.reshape(got[k].shape) for k, v in want.items()}
    check(f"midas small decoder {name}", "decoder/" + name, golden, case, got, want)


def test_decoder_map_gradients_of_a_batch_are_its_images_one_by_one(solver, decoder_runs):
    case, gy, y, _saved, (_gw, _gb, gm) = decoder_runs["f256_96x64b2"]
    for b in range(case["maps"][0].shape[0]):
        maps = [m[b:b + 1] for m in case["maps"]]
        y1, saved1 = solver.midas_decoder_train(maps, case["weights"], case["biases"], non_negative=case["non_negative"])
        assert (y1 == y[b:b + 1]).all()
        _w, _b, gm1 = solver.midas_decoder_backward(gy[b:b + 1], maps, saved1, case["weights"], case["biases"], non_negative=case["non_negative"])
        assert all((a == g[b:b + 1]).all() for a, g in zip(gm1, gm)), b


def test_decoder_refusals(solver, decoder_runs):
    case, gy, _y, saved, _grads = decoder_runs["f256_64x96"]
    args = (case["maps"], saved, case["weights"], case["biases"])
    with pytest.raises(ValueError, match="gy must be"):
        solver.midas_decoder_backward(gy[:, :-1], *args)
    with pytest.raises(ValueError, match="saved table"):
        solver.midas_decoder_backward(gy, case["maps"], saved[:-1], case["weights"], case["biases"])
    with pytest.raises(TypeError):
        solver.midas_decoder_backward(gy.astype(np.float64), *args)
    with pytest.raises(ValueError):
        solver.midas_decoder_train(case["maps"][:3], case["weights"], case["biases"])
    lib, h = api.load_library(), solver._h
    i32, four = C.c_int32, C.c_int32 * 4
    with api._DeviceArrays() as dev:
        buf, apart = dev.alloc(1 << 20), dev.alloc(1 << 20)
        t4, t16, t17, t21 = ((C.c_void_p * n)(*([buf.value] * n)) for n in (4, 16, 17, 21))
        sizes = (four(16, 16, 16, 16), four(8, 4, 2, 1), four(8, 4, 2, 1))
        bad_sizes = (four(16, 16, 16, 16), four(8, 4, 2, 1), four(8, 4, 3, 1))
        hole = (C.c_void_p * 16)(*([buf.value] * 15 + [None]))

        def train(feat=16, dims=sizes, nn=1, saved=t16, out=apart):
            return lib.cvd_midas_decoder_train_device(h, i32(1), i32(feat), *dims, t4, t21, t17, i32(nn), saved, out, None)

        def back(feat=16, dims=sizes, nn=1, gy=buf, saved=t16, gw=t21):
            return lib.cvd_midas_decoder_backward_device(h, i32(1), i32(feat), *dims, gy, t4, saved, t21, t17, i32(nn), gw, t17, None, None)
        for call, word in ((lambda: train(saved=None), b"null saved table"), (lambda: train(saved=hole), b"null saved tensor"),
                           (lambda: train(feat=0), b"features"), (lambda: train(dims=bad_sizes), b"not twice"), (lambda: train(nn=2), b"non_negative"),
                           (lambda: train(), b"overlaps"),
                           (lambda: back(gy=None), b"null"), (lambda: back(saved=hole), b"null saved tensor"), (lambda: back(feat=0), b"features"),
                           (lambda: back(dims=bad_sizes), b"not twice"), (lambda: back(nn=2), b"non_negative"), (lambda: back(gw=None), b"null")):
            assert call() != 0
            assert word in lib.cvd_last_error(h), (word, lib.cvd_last_error(h))
        assert api._hip_runtime().hipDeviceSynchronize() == 0


def test_torch_modules():
    """robust_cvd_amd.midas_train on GPU tensors, in a fresh process: torch has to be imported before libcvd_hip.so is loaded.  The
    checks are tests/midas_grad_torch_child.py's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.midas_grad_torch_child"], cwd=root, capture_output=True, text=True, timeout=300)
    print(r.stdout[-8000:])
    assert r.returncode == 0 and "midas train modules ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_refusals(solver):
    """Before any device work, with an error that names the value."""
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(TypeError):
        solver.midas_conv_grad_input(z(1, 8, 4, 4).astype(np.float64), z(8, 4, 3, 3))
    with pytest.raises(TypeError):
        solver.midas_conv_grad_weight(z(1, 8, 4, 4), z(1, 4, 4, 4).astype(np.float16), 3)
    with pytest.raises(TypeError):
        solver.midas_upsample2x_grad(z(1, 2, 4, 4).astype(np.float64))
    with pytest.raises(ValueError, match="filter"):
        solver.midas_conv_grad_weight(z(1, 8, 4, 4), z(1, 4, 4, 4), 5)
    with pytest.raises(ValueError, match="split"):
        solver.midas_conv_grad_input(z(1, 8, 4, 4), z(8, 4, 3, 3), split=2)
    # the C ABI's own checks
    lib, h = api.load_library(), solver._h
    i32 = C.c_int32
    with api._DeviceArrays() as dev:
        a = dev.alloc(4 * 8 * 16 * 9)
        b = dev.alloc(4 * 8 * 16 * 9)
        g = dev.alloc(4 * 8 * 16 * 9)

        def dgrad(B=1, H=4, W=4, cin=4, n=8, k=3, gy=a, w=b, add=None, mask=None, split=0, gx=g):
            return lib.cvd_midas_conv_grad_input_device(h, i32(B), i32(H), i32(W), i32(cin), i32(n), i32(k), gy, w, add, mask, i32(split), gx, None)

        def wgrad(B=1, H=4, W=4, cin=4, n=8, k=3, gy=a, x=b, relu_in=0, split=0, gw=g, gb=None):
            return lib.cvd_midas_conv_grad_weight_device(h, i32(B), i32(H), i32(W), i32(cin), i32(n), i32(k), gy, x, i32(relu_in), i32(split), gw, gb, None)

        def up(B=1, c=2, H=2, W=2, align=1, gy=a, gx=g):
            return lib.cvd_midas_upsample2x_grad_device(h, i32(B), i32(c), i32(H), i32(W), i32(align), gy, gx, None)
        hx, hw2, hb2, hw4, hb4, hgy = (dev.alloc(n) for n in (4 * 128 * 16, 4 * 32 * 128 * 9, 4 * 32, 4 * 32, 4, 4 * 16))
        ho = [dev.alloc(n) for n in (4 * 128 * 16, 4 * 32 * 128 * 9, 4 * 32, 4 * 32, 4)]

        def hgrad(B=1, H=4, W=4, cin=128, mid=32, gy=hgy, x=hx, nn=1, outs=ho):
            return lib.cvd_midas_head_grad_device(h, i32(B), i32(H), i32(W), i32(cin), i32(mid), gy, x, hw2, hb2, hw4, hb4, i32(nn), *outs, None)
        assert dgrad() == 0 and wgrad() == 0 and up() == 0 and hgrad() == 0
        for call, word in ((lambda: hgrad(W=0), b">= 1"), (lambda: hgrad(mid=16), b"mid_channels"), (lambda: hgrad(nn=3), b"non_negative"),
                           (lambda: hgrad(x=None), b"null"), (lambda: hgrad(outs=[hx] + ho[1:]), b"overlaps an input"),
                           (lambda: hgrad(outs=[ho[0], ho[1], ho[2], ho[2], ho[4]]), b"overlap")):
            assert call() != 0
            assert word in lib.cvd_last_error(h), (word, lib.cvd_last_error(h))
        for call, word in ((lambda: dgrad(B=0), b">= 1"), (lambda: dgrad(k=2), b"kernel_size"), (lambda: dgrad(cin=0), b"in_channels"),
                           (lambda: dgrad(split=2), b"split"), (lambda: dgrad(split=-1), b"split"), (lambda: dgrad(gy=None), b"null"),
                           (lambda: dgrad(gx=a), b"overlaps gy"), (lambda: dgrad(gx=b), b"overlaps the weight"),
                           (lambda: dgrad(add=g), b"overlaps the addend"), (lambda: dgrad(mask=g), b"overlaps the mask"),
                           (lambda: wgrad(H=0), b">= 1"), (lambda: wgrad(k=5), b"kernel_size"), (lambda: wgrad(n=0), b"out_channels"),
                           (lambda: wgrad(relu_in=2), b"relu_in"), (lambda: wgrad(split=129), b"split"), (lambda: wgrad(x=None), b"null"),
                           (lambda: wgrad(gw=a), b"overlaps an input"), (lambda: wgrad(gb=b), b"overlaps an input"),
                           (lambda: wgrad(gb=g), b"two gradients overlap"),
                           (lambda: up(c=0), b">= 1"), (lambda: up(align=2), b"align_corners"), (lambda: up(gx=None), b"null"),
                           (lambda: up(gx=a), b"overlaps gy")):
            assert call() != 0
            assert word in lib.cvd_last_error(h), (word, lib.cvd_last_error(h))
        assert api._hip_runtime().hipDeviceSynchronize() == 0
