"""CPU checks of the update-block fixture (tests/golden/reference_py/raftblock_golden.npz, minted from the reference's
BasicUpdateBlock and its layers' function by make_raftblock_golden.py): the float64 restatement the GPU tests measure against
(tests/raftblock_reference.py) reproduces the reference's stored f32 outputs within the reference's own recorded error, the
generators still build the inputs the fixture was minted from, the planted case is exact in double, where the reference checkout
is mounted it agrees with the restatement, the Python layers' domain checks raise without a device, and the torch module carries
the reference's state-dict keys."""
import numpy as np
import pytest

from tests import raftblock_cases as bc
from tests import raftblock_reference as br


@pytest.fixture(scope="module")
def golden():
    return np.load(br.GOLDEN)


@pytest.fixture(scope="module")
def restated():
    """Per case: (inputs, dict of f64 outputs): computed once, shared, left unchanged."""
    out = {}
    for name in bc.CONV_CASES:
        case = bc.make_conv_case(name)
        out["conv/" + name] = (case, {"out": br.conv_case(case)})
    for name in bc.BLOCK_CASES:
        case = bc.make_block_case(name)
        net, mask, delta_flow, kept = br.block_case(case, details=True)
        out["block/" + name] = (case, {"net": net, "mask": mask, "delta_flow": delta_flow, **kept})
    return out


ALL = ["conv/" + n for n in bc.CONV_CASES] + ["block/" + n for n in bc.BLOCK_CASES]


def outputs_of(key):
    return bc.OUTPUTS if key.startswith("block/") else ("out",)


@pytest.mark.parametrize("key", ALL)
def test_inputs_are_the_minted_ones(restated, golden, key):
    case = restated[key][0]
    assert bc.input_digest(case) == golden[key + "/input_sha256"].tobytes().decode()
    B, _, H, W = (case["net"] if key.startswith("block/") else case["x"]).shape
    most = bc.BLOCK_MAX_SAMPLES if key.startswith("block/") else bc.CONV_MAX_SAMPLES
    s = golden[key + "/samples"]
    assert np.array_equal(s, case["samples"]) and len(s) == min(B * H * W, most) <= 64
    assert {0, W - 1, (H - 1) * W, H * W - 1, B * H * W - 1} <= set(s.tolist())


@pytest.mark.parametrize("key", ALL)
def test_restatement_reproduces_the_reference(restated, golden, key):
    case, outs = restated[key]
    for o in outputs_of(key):
        out = outs[o]
        assert np.isfinite(out).all()
        stored = golden[f"{key}/{o}"]
        assert stored.shape == (len(case["samples"]), out.shape[1]) and stored.dtype == np.float32
        delta, scale = float(golden[f"{key}/{o}_delta"]), float(golden[f"{key}/{o}_scale"])
        err = np.abs(stored - bc.sample_view(case, out)).max()
        assert err <= delta, (o, err, delta)
        assert np.abs(out).max() == scale
        # the reference's own f32 error is a rounding error: a handful of ulps of the scale
        assert delta <= 64 * br.EPS32 * scale, (o, delta, scale)


def test_the_cases_cover_the_layer_shapes(restated):
    shapes = {(c["k"], c["segments"], c["weights"][0].shape[0], len(c["weights"])) for k, (c, _o) in restated.items() if k.startswith("conv/")}
    assert shapes == {(1, (324,), 256, 1), (3, (192, 64), 126, 1), (7, (2,), 128, 1), (3, (256,), 2, 1), (3, (128,), 256, 2),
                      (1, (256,), 576, 1)}
    case = restated["conv/c1s_1x4x6"][0]
    assert case["scale"] == 0.25 and not case["relu"]
    assert [tuple(w.shape) for w in restated["block/9x11"][0]["weights"]] == \
        [(o, c) + ((k, k) if isinstance(k, int) else k) for _n, o, c, k in bc.LAYERS]


def test_planted_is_exact_in_double(restated):
    case, outs = restated["block/planted"]
    where = {"encoder.convc1": ("cor1", 0), "encoder.convc2": ("cor_flo", 0), "encoder.convf1": ("flo1", 0),
             "encoder.convf2": ("cor_flo", 192), "encoder.conv": ("motion_features", 0), "flow_head.conv1": ("flow_hidden", 0),
             "flow_head.conv2": ("delta_flow", 0), "mask.0": ("mask_hidden", 0), "mask.2": ("mask", 0)}
    for layer, (zeroed, minus) in bc.PLANTED.items():
        tensor, first = where[layer]
        for ch, value in zeroed.items():
            b = float(np.float32(value))
            want = {"flow_head.conv2": b, "mask.2": 0.25 * b}.get(layer, max(b, 0.0))
            assert (outs[tensor][:, first + ch] == want).all(), (layer, ch)
        for ch in minus:
            assert (outs[tensor][:, first + ch] == 0.0).all(), (layer, ch)
    assert np.array_equal(outs["motion_features"][:, 126:], case["flow"].astype(np.float64))


def test_the_border_scaling_shows_a_leaked_halo(restated):
    """Pixel (0, 0) of image 1 differs when image 0's last row is its halo: the images stacked into one tall image."""
    case, outs = restated["conv/c3seg_3x5x7"]
    tall = dict(case, x=np.concatenate(list(case["x"]), 1)[None])
    assert np.abs(br.conv_case(tall)[0, :, 5, 0] - outs["out"][1, :, 0, 0]).max() > 1e-3


def test_live_reference_agrees(restated, golden):
    ref = br.load_reference()
    if ref is None:
        pytest.skip("the reference checkout (or torch) is not available here")
    assert list(ref(br.Args(), hidden_dim=128, input_dim=128).state_dict().keys()) == golden["state_dict_keys"].tolist()
    for name in ("9x11", "3x2"):
        case, outs = restated["block/" + name]
        for o, out32 in zip(bc.OUTPUTS, br.reference_block_output(ref, case)):
            # torch's CPU convolution may pick another summation order on another machine: another f32 evaluation of the same
            # formulas, held to the bar the kernel is held to
            assert np.abs(out32 - outs[o]).max() <= br.bar(golden[f"block/{name}/{o}_delta"], golden[f"block/{name}/{o}_scale"]), (name, o)


def test_domain_checks_need_no_device():
    from robust_cvd_amd import api
    assert api.UPDATE_BLOCK_PARAMETERS == bc.PARAMETERS and api.RAFT_COR_PLANES == bc.COR_PLANES
    w = [api.raft_block_weight_shape(n) for n in api.UPDATE_BLOCK_PARAMETERS]
    assert w == [(o, c) + ((k, k) if isinstance(k, int) else k) for _n, o, c, k in bc.LAYERS]
    b = [(s[0],) for s in w]
    good = ((2, 128, 9, 11), (2, 128, 9, 11), (2, 324, 9, 11), (2, 2, 9, 11), w, b)
    assert api.raft_check_update_block(*good) == (2, 9, 11)
    w196 = [api.raft_block_weight_shape(n, 196) for n in api.UPDATE_BLOCK_PARAMETERS]
    assert api.raft_check_update_block((1, 128, 3, 2), (1, 128, 3, 2), (1, 196, 3, 2), (1, 2, 3, 2), w196, b) == (1, 3, 2)

    def but(i, v):
        return good[:i] + (v,) + good[i + 1:]
    refused = [but(0, (2, 96, 9, 11)), but(0, (128, 9, 11)), but(1, (2, 256, 9, 11)), but(1, (2, 128, 9, 12)),
               but(2, (2, 196, 9, 11)),                     # corr channels that differ from convc1's Cin
               but(2, (1, 324, 9, 11)), but(3, (2, 3, 9, 11)), but(3, (2, 2, 11, 9)),
               ((0, 128, 9, 11), (0, 128, 9, 11), (0, 324, 9, 11), (0, 2, 9, 11), w, b),          # B H W = 0
               ((2, 128, 0, 11), (2, 128, 0, 11), (2, 324, 0, 11), (2, 2, 0, 11), w, b),
               but(4, w[:14]), but(4, w[::-1]), but(4, w[:4] + [(126, 256, 5, 5)] + w[5:]), but(5, [(64,)] * 15)]
    for args in refused:
        with pytest.raises(ValueError):
            api.raft_check_update_block(*args)

    x = (3, 5, 7)
    assert api.raft_check_conv2d([(3, 324) + x[1:]], [(256, 324, 1, 1)], [(256,)]) == (3, 5, 7, 256)
    assert api.raft_check_conv2d([(3, 192) + x[1:], (3, 64) + x[1:]], [(126, 256, 3, 3)], [(126,)], 128, 0) == (3, 5, 7, 126)
    assert api.raft_check_conv2d([(3, 128) + x[1:]], [(256, 128, 3, 3)] * 2, [(256,)] * 2) == (3, 5, 7, 512)
    assert api.raft_check_conv2d([(1, 2, 1, 1)], [(128, 2, 7, 7)], [(128,)]) == (1, 1, 1, 128)
    assert api.raft_check_conv2d([(3, 128) + x[1:]], [(64, 128, 3, 3)], [(64,)], 256, 192) == (3, 5, 7, 64)
    refused = [
        dict(segment_shapes=[(3, 256, 5, 7)], weight_shapes=[(126, 256, 5, 5)], bias_shapes=[(126,)]),          # filter size
        dict(segment_shapes=[(3, 256, 5, 7)], weight_shapes=[(126, 256, 3, 1)], bias_shapes=[(126,)]),
        dict(segment_shapes=[(3, 256, 5, 7)], weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(126,)], stride=2),
        dict(segment_shapes=[(3, 256, 5, 7)], weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(126,)], dilation=(2, 2)),
        dict(segment_shapes=[(3, 256, 5, 7)], weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(126,)], groups=2),
        dict(segment_shapes=[(0, 256, 5, 7)], weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(126,)]),          # B H W = 0
        dict(segment_shapes=[(3, 64, 5, 7)] * 4, weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(126,)]),       # > 3 segments
        dict(segment_shapes=[], weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(126,)]),
        dict(segment_shapes=[(3, 100, 5, 7), (3, 156, 5, 7)], weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(126,)]),
        dict(segment_shapes=[(3, 192, 5, 7), (3, 64, 5, 8)], weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(126,)]),
        dict(segment_shapes=[(3, 192, 5, 7)], weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(126,)]),          # Cin mismatch
        dict(segment_shapes=[(3, 256, 5, 7)], weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(128,)]),
        dict(segment_shapes=[(3, 256, 5, 7)], weight_shapes=[(126, 256, 3, 3)] * 2, bias_shapes=[(126,)] * 2),  # stacked, not x 64
        dict(segment_shapes=[(3, 256, 5, 7)], weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(126,)], out_channels_total=128, out_first=3),
        dict(segment_shapes=[(3, 256, 5, 7)], weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(126,)], out_channels_total=100),
        dict(segment_shapes=[(3, 256, 5, 7)], weight_shapes=[(126, 256, 3, 3)], bias_shapes=[(126,)], out_first=-1),
    ]
    for kwargs in refused:
        with pytest.raises(ValueError):
            api.raft_check_conv2d(**kwargs)


def test_the_array_layer_refuses_before_it_touches_a_device():
    """Solver.raft_conv2d's and raft_update_block's own checks come before their first device call: a stand-in `self` without a
    handle is enough."""
    from robust_cvd_amd.api import Solver
    case = bc.make_block_case("1x1")
    args = [case[k] for k in ("net", "inp", "corr", "flow")]
    with pytest.raises(TypeError, match="float32"):
        Solver.raft_update_block(None, args[0].astype(np.float64), *args[1:], case["weights"], case["biases"])
    with pytest.raises(TypeError, match="float32"):
        Solver.raft_update_block(None, *args, [w.astype(np.float16) for w in case["weights"]], case["biases"])
    with pytest.raises(ValueError, match="encoder.convc1 takes 324"):
        Solver.raft_update_block(None, args[0], args[1], args[2][:, :196], args[3], case["weights"], case["biases"])
    with pytest.raises(ValueError, match="B H W = 0"):
        Solver.raft_update_block(None, *(a[:0] for a in args), case["weights"], case["biases"])
    conv = bc.make_conv_case("c3seg_1x3x2")
    with pytest.raises(TypeError, match="float32"):
        Solver.raft_conv2d(None, conv["x"].astype(np.float64), conv["weights"][0], conv["biases"][0])
    with pytest.raises(ValueError, match="multiple of 32"):
        Solver.raft_conv2d(None, (conv["x"][:, :100], conv["x"][:, 100:]), conv["weights"][0], conv["biases"][0])
    with pytest.raises(ValueError, match="exceeds"):
        Solver.raft_conv2d(None, conv["x"], conv["weights"][0], conv["biases"][0], out=np.zeros((1, 128, 3, 2), np.float32), out_first=3)


def test_the_module_has_the_reference_state_dict_keys():
    """raft_ops.BasicUpdateBlock's state-dict keys equal the recorded keys of the reference's module and a case's state dict loads
    strictly.  In a fresh process (tests/raftblock_torch_child.py --keys; no GPU is touched): torch has to be imported before
    libcvd_hip.so is loaded, and this process may hold the library already."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.raftblock_torch_child", "--keys"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "raft block state dict keys ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
