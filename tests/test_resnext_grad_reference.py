"""CPU checks around the backbone's training operators: the float64 restatement (tests/resnext_grad_reference.py)
against the fixture minted from stock torch autograd, the condition against a vacuous bar, the adjoint identities on planted
integers, the split rules of csrc/cvd_resnext_grad.h against their mirrors in api.py, and the shape refusals.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from robust_cvd_amd import api
from tests import resnext_grad_cases as gc
from tests import resnext_grad_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robust_cvd_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def golden():
    return np.load(gr.GOLDEN)


def wanted(kind, name):
    if kind == "norm":
        case = gc.make_norm_case(name)
        fwd, bwd = gr.norm_case(case)
        want = {"y": fwd[0], "running_mean": fwd[3], "running_var": fwd[4], "gc": bwd[0], "g_gamma": bwd[1], "g_beta": bwd[2]}
        if case["residual"] is not None:
            want["g_residual"] = bwd[3]
    elif kind == "grouped":
        case = gc.make_grouped_case(name)
        want = dict(zip(("gx", "gw"), gr.grouped_case(case)))
    elif kind == "dense":
        case = gc.make_dense_case(name)
        want = dict(zip(("gx", "gw"), gr.dense_case(case)))
    elif kind == "block":
        case = gc.make_block_case(name)
        want = gr.block_case(case)
    else:
        case = gc.make_pool_case(name)
        want = {"gx": gr.maxpool_grad(case["x"], case["gy"])}
    return case, want


ALL = [("norm", n) for n in gc.NORM_CASES] + [("grouped", n) for n in gc.GROUPED_CASES] + [("dense", n) for n in gc.DENSE_CASES] \
    + [("pool", n) for n in gc.POOL_CASES] + [("block", n) for n in gc.BLOCK_CASES]


@pytest.mark.parametrize("kind,name", ALL)
def test_the_restatement_is_what_stock_torch_computes(golden, kind, name):
    """every tensor: the case is the minted one, torch's stored f32 values lie delta from the restatement, and delta <= 1e-4 scale
    (a draw that misses it would make the GPU bar vacuous and is replaced)"""
    case, want = wanted(kind, name)
    key = f"{kind}/{name}"
    assert gc.input_digest(case) == golden[f"{key}/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    for tensor, ref in want.items():
        delta, scale = float(golden[f"{key}/{tensor}_delta"]), float(golden[f"{key}/{tensor}_scale"])
        assert scale == float(np.abs(ref).max())
        assert delta <= 1e-4 * scale, (key, tensor, delta, scale)
        if f"{key}/{tensor}" in golden.files:
            assert float(np.abs(golden[f"{key}/{tensor}"] - ref).max()) == delta
        else:
            assert ref.size > gr.STORED_ELEMENTS
        if name.startswith("planted"):
            assert delta == 0.0, (key, tensor)


def test_the_fixture_is_small():
    assert os.path.getsize(gr.GOLDEN) < 1_000_000


@pytest.mark.parametrize("kind,name", [(k, n) for k, n in ALL if n.startswith("planted")])
def test_adjoint_identities_hold_exactly_on_planted_integers(kind, name):
    """<gy, conv(u)> = <dgrad(gy), u> = <wgrad(gy, u), W>: small integers, exact in double"""
    case = gc.make_grouped_case(name) if kind == "grouped" else gc.make_dense_case(name)
    groups = case.get("groups", 1)
    gx, gw = gr.conv_grads(case["gy"], case["x"], case["weight"], case["stride"], groups)
    y = gr.conv_forward(case["x"], case["weight"], case["stride"], groups)
    a = float((case["gy"].astype(np.float64) * y).sum())
    assert a == float((gx * case["x"]).sum()) == float((gw * case["weight"]).sum())


def test_strided_pointwise_input_gradient_is_zero_at_the_odd_positions():
    for name in ("k1_s2_5x7", "k1_s2_70_130_9x9", "planted_k1_s2_5x6"):
        gx, _ = gr.dense_case(gc.make_dense_case(name))
        mask = np.ones(gx.shape[2:], bool)
        mask[::2, ::2] = False
        assert (gx[:, :, mask] == 0).all() and (gx[:, :, ::2, ::2] != 0).any()


def test_pool_cases_hold_what_they_are_for():
    relu = gc.make_pool_case("relu_7x9")
    assert (relu["x"] == 0).mean() >= 0.4
    four = gc.make_pool_case("four_windows_5x5")
    gx = gr.maxpool_grad(four["x"], four["gy"])
    assert gx[0, 0, 1, 1] == four["gy"][0, 0, 0:2, 0:2].astype(np.float64).sum()         # the argmax of four windows
    equal = gc.make_pool_case("all_equal_6x10")
    gx = gr.maxpool_grad(equal["x"], equal["gy"])
    assert gx[0, 0, 0, 0] == equal["gy"][0, 0, 0, 0] and gx[0, 0, 1, 1] == equal["gy"][0, 0, 1, 1]   # the first of equal values


def test_block_saved_table():
    """api.resnext_block_saved_shapes: per convolution c, mean, invstd and the post-activation tensor; entry 11 is the output"""
    shapes = api.resnext_block_saved_shapes(2, 5, 7, 256, 64, 512, 2, True)
    assert shapes == [(2, 64, 5, 7), (64,), (64,), (2, 64, 5, 7), (2, 64, 3, 4), (64,), (64,), (2, 64, 3, 4),
                      (2, 512, 3, 4), (512,), (512,), (2, 512, 3, 4), (2, 512, 3, 4), (512,), (512,), (2, 512, 3, 4)]
    assert len(api.resnext_block_saved_shapes(1, 6, 6, 256, 32, 256)) == 12
    for name in gc.BLOCK_CASES:
        case = gc.make_block_case(name)
        dims = api.resnext_check_block(case["x"].shape, [w.shape for w in case["weights"]], [[a.shape for a in four] for four in case["norms"]],
                                       case["stride"], training=case["training"])
        assert dims[6] == case["groups"] and dims[8] == (len(case["weights"]) == 4)
    with pytest.raises(ValueError):                  # no downsample branch at stride 2
        api.resnext_check_block((1, 256, 6, 6), [(32, 256, 1, 1), (32, 8, 3, 3), (256, 32, 1, 1)], [[(32,)] * 4, [(32,)] * 4, [(256,)] * 4], 2)
    with pytest.raises(ValueError):                  # 12 channels per group are not built
        api.resnext_check_block((1, 256, 6, 6), [(48, 256, 1, 1), (48, 12, 3, 3), (256, 48, 1, 1)], [[(48,)] * 4, [(48,)] * 4, [(256,)] * 4])
    # everything saved, nothing recomputed: the whole ResNeXt-101 32x8d at one 384 x 224 frame
    total = api.resnext_saved_bytes(224, 384)
    assert 300e6 < total < 450e6, total
    assert api.resnext_saved_bytes(224, 384, batch=8) > 7.9 * total


def test_norm_split_rule():
    for name, S in gc.EXPECTED_NORM_SPLIT.items():
        B, N, H, W = gc.NORM_CASES[name][0]
        assert api.resnext_norm_split(N, B * H * W) == S, name
    # the stem at 384 x 224: 64 channels over 21 504 B values each get several slices
    assert api.resnext_norm_split(64, 21504) == 11 and api.resnext_norm_split(64, 8 * 21504) == 16
    assert api.resnext_norm_split(2048, 84) == 1
    for N in (1, 3, 64, 256, 2048):
        last = 1
        for M in (2, 1024, 1025, 5000, 21504, 172032, 10 ** 7):
            S = api.resnext_norm_split(N, M)
            chunks = -(-M // api.RESNEXT_NORM_CHUNK)
            assert 1 <= S <= min(chunks, api.RESNEXT_NORM_MAX_SPLIT) and (S - 1) * -(-chunks // S) < chunks
            assert S >= last
            last = S


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_python_rules_are_the_headers(tmp_path):
    """rxgNormSplit and rxgWgradSplit of csrc/cvd_resnext_grad.h, compiled for the host, against their mirrors in api.py"""
    norm = [(N, M) for N in (1, 3, 64, 256, 2048) for M in (2, 1024, 1025, 4800, 21504, 172032, 10 ** 7)]
    wgrad = [(M, E) for M in (1, 35, 256, 257, 312, 5376, 43008, 344064) for E in (72, 9408, 18432, 147456, 589824)]
    src = tmp_path / "split.hip"
    src.write_text(f'#include <cstdio>\n#include "{CSRC}/cvd_resnext_grad.h"\nint main() {{\n'
                   + "".join(f'  std::printf("%d\\n", cvd::rxgNormSplit({N}ll, {M}ll));\n' for N, M in norm)
                   + "".join(f'  std::printf("%d\\n", cvd::rxgWgradSplit({M}ll, {E}ll));\n' for M, E in wgrad) + "  return 0;\n}\n")
    exe = tmp_path / "split"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", str(exe), str(src)], check=True, capture_output=True, timeout=300)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [api.resnext_norm_split(N, M) for N, M in norm] + [api.resnext_wgrad_split(M, E) for M, E in wgrad]
    G, cg, stride, (B, H, W), split = gc.GROUPED_CASES["g4x8_s1_12x13b2_split2"]
    assert api.resnext_wgrad_split(B * H * W, G * cg * cg * 9) == 2 == split       # the rule cuts this case's pixels too


def test_the_shape_checks_refuse_before_any_device_work():
    four = [(5,)] * 4
    for bad in (lambda: api.resnext_check_norm_train((1, 5, 1, 1), four),                        # one value per channel in training
                lambda: api.resnext_check_norm_train((2, 5, 3, 7), four, momentum=None),
                lambda: api.resnext_check_norm_train((2, 5, 3, 7), four, momentum=1.5),
                lambda: api.resnext_check_norm_train((2, 5, 3, 7), four, eps=0.0),
                lambda: api.resnext_check_norm_train((2, 5, 3, 7), [(4,)] * 4),
                lambda: api.resnext_check_norm_train((2, 5, 3, 7), four, residual_shape=(2, 5, 3, 6)),
                lambda: api.resnext_check_norm_grad((2, 5, 3, 7), (2, 5, 3, 6), None, [(5,)] * 3),
                lambda: api.resnext_check_norm_grad((2, 5, 3, 7), (2, 5, 3, 7), None, [(5,)] * 2),
                lambda: api.resnext_check_grouped_conv_grad_input((1, 32, 3, 3), (32, 8, 3, 3), (5, 7), 2),   # gy is 3 x 4 for 5 x 7
                lambda: api.resnext_check_grouped_conv_grad_input((1, 32, 5, 7), (32, 12, 3, 3), (5, 7)),     # 12 per group: not built
                lambda: api.resnext_check_grouped_conv_grad_input((1, 32, 5, 7), (32, 8, 3, 3), (5, 7), 3),
                lambda: api.resnext_check_grouped_conv_grad_weight((1, 32, 5, 7), (1, 32, 5, 7), 8, split=129),
                lambda: api.resnext_check_grouped_conv_grad_weight((1, 32, 5, 7), (1, 24, 5, 7), 8),
                lambda: api.resnext_check_conv_grad_input((1, 64, 5, 6), (64, 3, 7, 7), (9, 11), 2),          # the stem's is not built
                lambda: api.resnext_check_conv_grad_input((1, 8, 5, 7), (8, 4, 1, 1), (5, 7), add_shape=(1, 8, 5, 7)),
                lambda: api.resnext_check_conv_grad_weight((1, 8, 5, 7), (1, 4, 5, 7), 3),
                lambda: api.resnext_check_conv_grad_weight((1, 8, 5, 7), (1, 4, 5, 7), 7, 1),
                lambda: api.resnext_check_maxpool_grad((1, 2, 5, 7), (1, 2, 3, 3))):
        with pytest.raises(ValueError):
            bad()
    assert api.resnext_check_norm_train((1, 5, 1, 1), four, training=False) == (1, 5, 1, 1)
    assert api.resnext_check_grouped_conv_grad_input((1, 32, 3, 4), (32, 8, 3, 3), (5, 7), 2) == (1, 5, 7, 4, 8)
    assert api.resnext_check_conv_grad_weight((2, 64, 5, 6), (2, 3, 9, 11), 7, 2) == (2, 9, 11, 3, 64, 7)
    assert api.resnext_check_maxpool_grad((1, 2, 5, 7), (1, 2, 3, 4)) == (1, 2, 5, 7)


CLASS_CHECK = '''
from robust_cvd_amd import api, midas, midas_train
try:
    midas_train.MidasNet(backbone=midas.ResNeXt((1, 1, 1, 1), 4, 8), features=8)
    raise SystemExit("the forward-only class was accepted")
except ValueError as e:
    assert "no kernel yet" in str(e) and "midas_train.ResNeXt" in str(e), e
net = midas_train.MidasNet(backbone=midas_train.ResNeXt((1, 1, 1, 1), 4, 8), features=8)
assert ["pretrained." + k for k in net.pretrained.state_dict()] == api.resnext_state_dict_keys((1, 1, 1, 1), 4, 8)
assert isinstance(net.pretrained.layer2[0], midas_train.Bottleneck) and isinstance(net.pretrained.layer2[0], midas.Bottleneck)
assert all(p.requires_grad for p in net.parameters())
assert len(midas_train.resnext101_32x8d().state_dict()) == 624
print("ok")
'''


def test_the_forward_only_class_is_still_refused_and_the_message_names_the_new_one():
    """(torch is imported first, in a process of its own; no GPU is touched: the classes are parameter holders until a forward)"""
    import sys
    pytest.importorskip("torch")
    done = subprocess.run([sys.executable, "-c", CLASS_CHECK], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and done.stdout.strip().endswith("ok"), done.stdout + done.stderr
