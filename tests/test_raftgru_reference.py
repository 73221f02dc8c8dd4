"""CPU checks of the SepConvGRU fixture (tests/golden/reference_py/raftgru_golden.npz, minted from the reference's SepConvGRU by
make_raftgru_golden.py): the float64 restatement the GPU tests measure against (tests/raftgru_reference.py) reproduces the
reference's stored f32 outputs within the reference's own recorded error, the generators still build the inputs the fixture was
minted from, where the reference checkout is mounted it agrees with the restatement, and the Python layers' domain checks raise
without a device."""
import numpy as np
import pytest

from tests import raftgru_cases as gc
from tests import raftgru_reference as gr


@pytest.fixture(scope="module")
def golden():
    return np.load(gr.GOLDEN)


@pytest.fixture(scope="module")
def restated():
    """Per case: (inputs, f64 output, per-half gates): computed once, shared, left unchanged."""
    out = {}
    for name in gc.CASES:
        case = gc.make_case(name)
        out[name] = (case,) + gr.sepconv_gru(case["h"], case["x"], case["weights"], case["biases"], details=True)
    return out


@pytest.mark.parametrize("name", list(gc.CASES))
def test_inputs_are_the_minted_ones(restated, golden, name):
    case = restated[name][0]
    assert gc.input_digest(case) == golden[name + "/input_sha256"].tobytes().decode()
    B, H, W = gc.CASES[name]
    s = golden[name + "/samples"]
    assert np.array_equal(s, case["samples"]) and len(s) == min(B * H * W, gc.MAX_SAMPLES)
    assert {0, W - 1, (H - 1) * W, H * W - 1, B * H * W - 1} <= set(s.tolist())
    assert golden[name + "/out"].shape == (len(s), gc.HIDDEN)


@pytest.mark.parametrize("name", list(gc.CASES))
def test_restatement_reproduces_the_reference(restated, golden, name):
    case, out, _gates = restated[name]
    assert out.shape == case["h"].shape and np.isfinite(out).all()
    err = np.abs(golden[name + "/out"] - gc.sample_view(case, out)).max()
    assert err <= float(golden[name + "/delta"]), (err, float(golden[name + "/delta"]))
    assert np.abs(out).max() == float(golden[name + "/scale"])
    # the reference's own f32 error is a rounding error: a handful of ulps of the scale
    assert float(golden[name + "/delta"]) <= 64 * gr.EPS32 * float(golden[name + "/scale"])


def test_the_cases_exercise_what_they_name(restated):
    # trained9x11: saturated gates
    _case, _out, gates = restated["trained9x11"]
    z1 = gates[0][0]
    assert (z1 < 1e-3).any() and (z1 > 1 - 1e-3).any()
    # pm100: planted gates are 0 / 1 to double precision, the output is h resp. +-1 there
    case, out, gates = restated["pm100"]
    for z, r, q in gates:
        assert z[:, list(gc.PLANTED["z"][0])].max() < 1e-40 and z[:, list(gc.PLANTED["z"][1])].min() == 1.0
        assert r[:, list(gc.PLANTED["r"][0])].max() < 1e-40 and r[:, list(gc.PLANTED["r"][1])].min() == 1.0
        assert (q[:, list(gc.PLANTED["q"][0])] == -1.0).all() and (q[:, list(gc.PLANTED["q"][1])] == 1.0).all()
    assert np.abs(out[:, list(gc.PM100_KEEPS_H)] - case["h"][:, list(gc.PM100_KEEPS_H)]).max() < 1e-40
    assert (out[:, list(gc.PM100_PLUS_ONE)] == 1.0).all() and (out[:, list(gc.PM100_MINUS_ONE)] == -1.0).all()
    # the border scaling shows in a zero-padded neighbourhood: pixel (0, 0) of image 1 differs when image 0's last row is its halo
    case = restated["5x7b3"][0]
    leaky = np.concatenate(list(case["h"]), 1)[None], np.concatenate(list(case["x"]), 1)[None]     # the images stacked: one tall image
    tall = gr.sepconv_gru(leaky[0], leaky[1], case["weights"], case["biases"])
    assert np.abs(tall[0, :, 5, 0] - restated["5x7b3"][1][1, :, 0, 0]).max() > 1e-3


def test_live_reference_agrees(restated, golden):
    ref = gr.load_reference()
    if ref is None:
        pytest.skip("the reference checkout (or torch) is not available here")
    for name, (case, out, _gates) in restated.items():
        out32 = gr.reference_output(ref, case)
        # torch's CPU convolution may pick another summation order on another machine: within twice the recorded error
        assert np.abs(out32 - out).max() <= 2 * float(golden[name + "/delta"]), name


def test_domain_checks_need_no_device():
    from robust_cvd_amd import api
    w = [api.raft_gru_weight_shape(n) for n in api.GRU_PARAMETERS]
    b = [(128,)] * 6
    assert [tuple(s) for s in w] == [gc.weight_shape(n) for n in gc.PARAMETERS] and api.GRU_PARAMETERS == gc.PARAMETERS
    assert api.raft_check_gru((2, 128, 9, 11), [(2, 256, 9, 11)], w, b) == (2, 9, 11)
    assert api.raft_check_gru((2, 128, 9, 11), [(2, 32, 9, 11), (2, 96, 9, 11), (2, 128, 9, 11)], w, b) == (2, 9, 11)
    refused = [
        ((2, 96, 9, 11), [(2, 256, 9, 11)], w, b),                       # hidden_dim
        ((2, 128, 9, 11), [(2, 320, 9, 11)], w, b),                      # input_dim
        ((2, 128, 9, 11), [(2, 128, 9, 11)], w, b),
        ((2, 128, 9, 11), [(2, 126, 9, 11), (2, 130, 9, 11)], w, b),     # segments not in multiples of 32
        ((2, 128, 9, 11), [(2, 64, 9, 11)] * 4, w, b),                   # too many segments
        ((2, 128, 9, 11), [], w, b),
        ((2, 128, 9, 11), [(2, 256, 9, 12)], w, b),
        ((2, 128, 9, 11), [(1, 256, 9, 11)], w, b),
        ((0, 128, 9, 11), [(0, 256, 9, 11)], w, b),                      # B H W = 0
        ((2, 128, 0, 11), [(2, 256, 0, 11)], w, b),
        ((128, 9, 11), [(256, 9, 11)], w, b),
        ((2, 128, 9, 11), [(2, 256, 9, 11)], w[::-1], b),                # 5 x 1 where 1 x 5 belongs
        ((2, 128, 9, 11), [(2, 256, 9, 11)], w[:5], b[:5]),
        ((2, 128, 9, 11), [(2, 256, 9, 11)], w, [(64,)] * 6),
    ]
    for args in refused:
        with pytest.raises(ValueError):
            api.raft_check_gru(*args)


def test_the_array_layer_refuses_before_it_touches_a_device():
    """Solver.raft_sepconv_gru's own checks come before its first device call: a stand-in `self` without a handle is enough."""
    from robust_cvd_amd.api import Solver
    case = gc.make_case("1x1")
    h, x, w, b = case["h"], case["x"], case["weights"], case["biases"]
    with pytest.raises(TypeError, match="float32"):
        Solver.raft_sepconv_gru(None, h.astype(np.float64), x, w, b)
    with pytest.raises(TypeError, match="float32"):
        Solver.raft_sepconv_gru(None, h, x.astype(np.float16), w, b)
    with pytest.raises(TypeError, match="float32"):
        Solver.raft_sepconv_gru(None, h, x, [a.astype(np.float64) for a in w], b)
    with pytest.raises(ValueError, match="multiple of 32"):
        Solver.raft_sepconv_gru(None, h, (x[:, :100], x[:, 100:]), w, b)
    with pytest.raises(ValueError, match="B H W = 0"):
        Solver.raft_sepconv_gru(None, h[:0], x[:0], w, b)
