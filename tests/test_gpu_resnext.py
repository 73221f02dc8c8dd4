"""GPU checks of the ResNeXt backbone kernels (robust_cvd_amd/csrc/cvd_resnext.h) through the array paths
(Solver.resnext_grouped_conv, resnext_conv, resnext_maxpool, midas_backbone) and, in a fresh process, through the torch drop-in
robust_cvd_amd.midas (tests/resnext_torch_child.py).

Bar: |kernel - f64| <= 8 x max(delta, 2^-23 x scale) against the float64 restatement (tests/resnext_reference.py), delta = stock
torch's own f32 error against that restatement for the case, scale = the largest |output|, both read from the fixture
(tests/golden/reference_py/resnext_golden.npz, minted on the CPU from stock torch modules wired as torchvision's; never from these
kernels); against the stored f32 values that bar + delta.  The planted cases are exact: ==."""
import os
import subprocess
import sys

import numpy as np
import pytest

from robust_cvd_amd import api
from tests import margins
from tests import resnext_cases as rc
from tests import resnext_reference as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    return api.Solver(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(rr.GOLDEN)


def run_grouped(solver, case, **over):
    c = dict(case, **over)
    return solver.resnext_grouped_conv(c["x"], c["weight"], stride=c["stride"], norm=c["norm"], eps=rc.EPS, relu=c["relu"])


def run_conv(solver, case, split=0, **over):
    c = dict(case, **over)
    return solver.resnext_conv(c["x"], c["weight"], stride=c["stride"], norm=c["norm"], eps=rc.EPS, relu=c["relu"], residual=c["residual"],
                               split=split)


def run_block(solver, x, params, stride):
    """A Bottleneck as the library chains it: conv1, the grouped conv2, downsample.0 where there is one, conv3 with the residual."""
    out = solver.resnext_conv(x, params[0][0], norm=params[0][1], relu=True)
    out = solver.resnext_grouped_conv(out, params[1][0], stride=stride, norm=params[1][1], relu=True)
    identity = x if len(params) == 3 else solver.resnext_conv(x, params[3][0], stride=stride, norm=params[3][1])
    return solver.resnext_conv(out, params[2][0], norm=params[2][1], residual=identity)


def chain(solver, case):
    """The backbone's stages one by one through the three entry points, as cvd_midas_backbone_device chains them."""
    p = case["params"]
    x = solver.resnext_maxpool(solver.resnext_conv(case["images"], p[0][0], stride=2, norm=p[0][1], relu=True))
    maps, at = [], 1
    for stage in range(4):
        for i in range(case["blocks"][stage]):
            n = 4 if i == 0 else 3
            x = run_block(solver, x, p[at:at + n], 2 if (stage > 0 and i == 0) else 1)
            at += n
        maps.append(x)
    return maps


def run_backbone(solver, case, **kw):
    return solver.midas_backbone(case["images"], [w for w, _ in case["params"]], [four for _, four in case["params"]], case["blocks"],
                                 case["groups"], case["width_per_group"], rc.EPS, **kw)


def check(label, key, golden, case, got, want, samples=None):
    assert rc.input_digest(case) == golden[f"{key}/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    delta = float(golden[f"{key}/out_delta"])
    bar = rr.bar(delta, golden[f"{key}/out_scale"])
    err = np.abs(got - want).max()
    print(f"{key}: max |kernel - f64| {err:.3e}, bar {bar:.3e}, share {err / bar if bar else 0.0:.3f} (stock torch's own delta {delta:.3e})")
    margins.below(label, err, bar)
    samples = case["samples"] if samples is None else samples
    margins.below(f"{label} vs reference", np.abs(rc.sample_view(got, samples) - golden[f"{key}/out"]).max(), bar + delta)


@pytest.fixture(scope="module")
def grouped_results(solver):
    """Per grouped case: (inputs, f64 restatement, kernel output): computed once, shared."""
    out = {}
    for name in rc.GROUPED_CASES:
        case = rc.make_grouped_case(name)
        out[name] = (case, rr.grouped_case(case), run_grouped(solver, case))
    return out


@pytest.fixture(scope="module")
def conv_results(solver):
    out = {}
    for name in rc.CONV_CASES:
        case = rc.make_conv_case(name)
        out[name] = (case, rr.conv_case(case), run_conv(solver, case))
    return out


@pytest.fixture(scope="module")
def backbone_results(solver):
    out = {}
    for name in rc.BACKBONE_CASES:
        case = rc.make_backbone_case(name)
        out[name] = (case, rr.backbone_case(case), run_backbone(solver, case))
    return out


@pytest.mark.parametrize("name", list(rc.GROUPED_CASES))
def test_grouped_conv_against_the_restatement_and_the_reference(grouped_results, golden, name):
    case, want, got = grouped_results[name]
    if name.startswith("planted"):
        assert (got == want).all() and (got == np.round(got)).all() and np.abs(got).max() > 20
    check(f"resnext grouped {name}", "grouped/" + name, golden, case, got, want)


def test_grouped_conv_keeps_the_groups_apart(solver):
    """perturbing the input channels of one group changes that group's output channels only: the rest is bit-identical"""
    for name, g in (("g32x8_s2_5x7b2", 17), ("g5x32_s1_3x5", 3), ("g2x64_s1_9x9b2", 0)):
        case = rc.make_grouped_case(name)
        cg = case["weight"].shape[1]
        base = run_grouped(solver, case)
        x = case["x"].copy()
        x[:, g * cg:(g + 1) * cg] += np.float32(1.5)
        got = run_grouped(solver, case, x=x)
        own = np.zeros(base.shape[1], bool)
        own[g * cg:(g + 1) * cg] = True
        assert np.array_equal(got[:, ~own], base[:, ~own]), name
        assert (got[:, own] != base[:, own]).mean() > 0.5, name


def test_grouped_conv_repeats_bit_for_bit_and_refuses(solver):
    case = rc.make_grouped_case("g32x8_s2_5x7b2")
    assert np.array_equal(run_grouped(solver, case), run_grouped(solver, case))
    with pytest.raises(ValueError, match=r"got 12"):
        solver.resnext_grouped_conv(np.zeros((1, 48, 5, 7), np.float32), np.zeros((48, 12, 3, 3), np.float32))
    with pytest.raises(ValueError, match="no whole groups|takes"):
        solver.resnext_grouped_conv(case["x"], np.zeros((256, 16, 3, 3), np.float32)[:, :12])
    with pytest.raises(TypeError, match="float32"):
        solver.resnext_grouped_conv(case["x"].astype(np.float64), case["weight"])
    # the library's own refusals, before any device work
    import ctypes as C
    fn = solver._fn("resnext_grouped_conv_device")
    args = [solver._h, C.c_int32(1), C.c_int32(5), C.c_int32(7), C.c_int32(4), C.c_int32(12), C.c_int32(1), C.c_void_p(256), C.c_void_p(512),
            None, C.c_float(1e-5), C.c_int32(0), C.c_void_p(1024), None]
    with pytest.raises(RuntimeError, match=r"8, 16, 32 or 64 \(got 12\)"):
        solver._check(fn(*args))
    args[5], args[6] = C.c_int32(8), C.c_int32(3)
    with pytest.raises(RuntimeError, match=r"stride must be 1 or 2 \(got 3\)"):
        solver._check(fn(*args))
    args[6], args[12] = C.c_int32(1), C.c_void_p(256)
    with pytest.raises(RuntimeError, match="out overlaps x"):
        solver._check(fn(*args))
    args[12], args[7] = C.c_void_p(1 << 20), None
    with pytest.raises(RuntimeError, match="null array"):
        solver._check(fn(*args))


@pytest.mark.parametrize("name", list(rc.POOL_CASES))
def test_maxpool_is_exact(solver, golden, name):
    case = rc.make_pool_case(name)
    got, want = solver.resnext_maxpool(case["x"]), rr.maxpool(case["x"])
    assert rc.input_digest(case) == golden[f"pool/{name}/input_sha256"].tobytes().decode()
    assert got.dtype == np.float32 and np.array_equal(got, want)             # a maximum of f32 values: no rounding
    assert np.array_equal(rc.sample_view(got, case["samples"]), golden[f"pool/{name}/out"])
    if name.startswith("negative"):
        assert (got[1] < 0).all() and (got[0] > 0).any()                      # a zero padding would have won


@pytest.mark.parametrize("name", list(rc.CONV_CASES))
def test_dense_conv_against_the_restatement_and_the_reference(conv_results, golden, name):
    case, want, got = conv_results[name]
    if name.startswith("planted"):
        assert (got == want).all() and (got == np.round(got)).all() and np.abs(got).max() > 20
    check(f"resnext conv {name}", "conv/" + name, golden, case, got, want)


@pytest.mark.parametrize("name", list(rc.SPLIT_CASES) + ["planted_512_40"])
def test_dense_conv_split_and_unsplit_both_hold_the_bar(solver, conv_results, golden, name):
    case, want, got = conv_results[name]
    cin, _cout, k, stride, (_B, H, W), _form = rc.CONV_CASES[name]
    S = api.resnext_split(cin * k * k, rc.out_size(H, stride) * rc.out_size(W, stride), k)
    assert S == rc.EXPECTED_SPLIT[name] and S > 1
    assert np.array_equal(run_conv(solver, case, split=S), got)               # the rule's S is what split = 0 ran
    assert np.array_equal(run_conv(solver, case), got)                        # and a call repeats bit for bit
    one = run_conv(solver, case, split=1)
    check(f"resnext conv {name} unsplit", "conv/" + name, golden, case, one, want)
    if name.startswith("planted"):
        assert np.array_equal(one, got) and np.array_equal(run_conv(solver, case, split=16), got)
    else:
        assert not np.array_equal(one, got)                                   # (another order of summation)


def test_dense_conv_refuses(solver):
    x = np.zeros((1, 8, 5, 7), np.float32)
    with pytest.raises(ValueError, match="kernel_size, stride"):
        solver.resnext_conv(x, np.zeros((4, 8, 3, 3), np.float32))
    with pytest.raises(ValueError, match="split must be 0"):
        solver.resnext_conv(x, np.zeros((4, 8, 1, 1), np.float32), split=2)
    import ctypes as C
    fn = solver._fn("resnext_conv_device")
    args = [solver._h, C.c_int32(1), C.c_int32(5), C.c_int32(7), C.c_int32(8), C.c_int32(4), C.c_int32(3), C.c_int32(1), C.c_void_p(256),
            C.c_void_p(8192), None, C.c_float(1e-5), C.c_int32(0), None, C.c_int32(0), C.c_void_p(1 << 20), None]
    with pytest.raises(RuntimeError, match=r"kernel_size must be 1 or 7 \(got 3\)"):
        solver._check(fn(*args))
    args[6] = C.c_int32(7)
    with pytest.raises(RuntimeError, match=r"stride 2 only \(got stride 1\)"):
        solver._check(fn(*args))
    args[6], args[14] = C.c_int32(1), C.c_int32(2)
    with pytest.raises(RuntimeError, match=r"split must be 0 \(the rule\) or 1 .. 1"):
        solver._check(fn(*args))
    args[14], args[2] = C.c_int32(0), C.c_int32(0)
    with pytest.raises(RuntimeError, match=r"must be >= 1 \(got 1, 0, 7\)"):
        solver._check(fn(*args))
    args[2] = C.c_int32(5)
    norm = (C.c_void_p * 4)(4096, 4096, 4096, 4096)
    args[10], args[11] = norm, C.c_float(0.0)
    with pytest.raises(RuntimeError, match="eps must be > 0"):
        solver._check(fn(*args))


@pytest.mark.parametrize("name", list(rc.BLOCK_CASES))
def test_bottleneck_against_the_restatement_and_the_reference(solver, golden, name):
    case = rc.make_block_case(name)
    assert (len(case["params"]) == 3) == (name == "identity")
    got = run_block(solver, case["x"], case["params"], case["stride"])
    check(f"resnext bottleneck {name}", "block/" + name, golden, case, got, rr.block_case(case))


@pytest.mark.parametrize("name", list(rc.BACKBONE_CASES))
def test_backbone_against_the_restatement_and_the_reference(backbone_results, golden, name):
    case, want, got = backbone_results[name]
    assert len(got) == 4
    for k in range(4):
        check(f"midas backbone {name} map {k + 1}", f"backbone/{name}/map{k + 1}", golden, case, got[k], want[k], case["samples"][k])


@pytest.mark.parametrize("name", list(rc.BACKBONE_CASES))
def test_backbone_equals_the_chained_entry_points_and_repeats(solver, backbone_results, name):
    case, _want, got = backbone_results[name]
    ms = []
    again = run_backbone(solver, case, kernel_ms=ms)
    chained = chain(solver, case)
    for k in range(4):
        assert np.array_equal(again[k], got[k]), (name, k)
        assert np.array_equal(chained[k], got[k]), (name, k)
    n = len(case["params"])
    assert len(ms) == 2 * n + 1 and all(ms[2 * i] > 0 for i in range(n)) and ms[2 * n] > 0
    table = api.resnext_conv_table(case["blocks"], case["groups"], case["width_per_group"])
    H, W = case["images"].shape[2:]
    for i, c in enumerate(table):                                             # a fold has a time exactly where the rule splits
        if c.groups > 1 or c.kernel_size == 7:
            assert ms[2 * i + 1] == 0
    assert any(ms[2 * i + 1] > 0 for i in range(n))                           # layer4's 1 x 1 convolutions split at these sizes


def test_backbone_refuses(solver):
    case = rc.make_backbone_case("small_32x32")
    with pytest.raises(ValueError, match="multiples of 32"):
        run_backbone(solver, dict(case, images=case["images"][:, :, :, :24]))
    with pytest.raises(ValueError, match="eps must be > 0"):
        solver.midas_backbone(case["images"], [w for w, _ in case["params"]], [f for _, f in case["params"]], *rc.SMALL, eps=0.0)
    import ctypes as C
    fn = solver._fn("midas_backbone_device")
    n = len(case["params"])
    ptrs = (C.c_void_p * n)(*([4096] * n))
    norms = (C.c_void_p * (4 * n))(*([4096] * (4 * n)))
    outs = (C.c_void_p * 4)(1 << 30, 1 << 31, 1 << 32, 1 << 33)

    def args(H=32, W=32, blocks=(2, 1, 2, 1), wpg=8, eps=1e-5, images=1 << 20, outs=outs, weights=ptrs):
        return [solver._h, C.c_int32(1), C.c_int32(H), C.c_int32(W), (C.c_int32 * 4)(*blocks), C.c_int32(4), C.c_int32(wpg), C.c_float(eps),
                C.c_void_p(images), weights, norms, outs, None]
    for kw, word in ((dict(W=48), r"multiples of 32 \(got 32 x 48\)"), (dict(blocks=(2, 0, 2, 1)), r"layer2 must be >= 1 \(got 0\)"),
                     (dict(wpg=12), r"layer1 has 12 channels per group"), (dict(eps=0.0), "eps must be > 0"), (dict(images=None), "null array"),
                     (dict(images=1 << 30), "output map 1 overlaps the images"),
                     (dict(outs=(C.c_void_p * 4)(1 << 30, 1 << 30, 1 << 32, 1 << 33)), "output map 2 overlaps output map 1"),
                     (dict(weights=(C.c_void_p * n)(*([4096] * (n - 1) + [None]))), f"null weight {n - 1}")):
        with pytest.raises(RuntimeError, match=word):
            solver._check(fn(*args(**kw)))


def test_torch_modules():
    """robust_cvd_amd.midas's Bottleneck, ResNeXt and MidasNet with the native backbone in a fresh process (torch first, then the
    library): tests/resnext_torch_child.py."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.resnext_torch_child"], cwd=root, capture_output=True, text=True, timeout=600)
    sys.stdout.write(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "resnext torch modules ok" in r.stdout
