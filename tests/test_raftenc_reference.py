"""CPU checks of the encoder tests' own parts (no GPU): the float64 restatement (tests/raftenc_reference.py) reproduces the
reference's stored f32 values within the stored delta, the seeded cases are the minted ones, the fixture is what the GPU tests
expect, and robust_cvd_amd.raft_ops.RAFT has the reference's state-dict keys (a child process: torch is imported there)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import raftenc_cases as ec
from tests import raftenc_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(er.GOLDEN)


def agree(golden, key, case, want, samples):
    assert ec.input_digest(case) == golden[f"{key}/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    delta = float(golden[f"{key}/out_delta"])
    stored = golden[f"{key}/out"]
    assert stored.dtype == np.float32
    # (the f64 matmul may round differently on another machine: a relative 1e-9 of slack, far below an f32 ulp)
    scale = float(golden[f"{key}/out_scale"])
    assert np.abs(ec.sample_view(want, samples) - stored).max() <= delta + 1e-9 * scale
    assert abs(scale - np.abs(want).max()) <= 1e-9 * scale
    # the reference's f32 arithmetic stays near the restatement: a delta far above f32 rounding would mean another formula
    assert delta <= 1e-3 * max(float(golden[f"{key}/out_scale"]), 1e-3), (key, delta)


@pytest.mark.parametrize("name", list(ec.CONV_CASES))
def test_convolution_restatement(golden, name):
    case = ec.make_conv_case(name)
    agree(golden, "conv/" + name, case, er.conv_case(case), case["samples"])


@pytest.mark.parametrize("name", list(ec.NORM_CASES))
def test_instance_norm_restatement(golden, name):
    case = ec.make_norm_case(name)
    agree(golden, "norm/" + name, case, er.norm_case(case), case["samples"])


@pytest.mark.parametrize("name", list(ec.ENCODER_CASES))
def test_encoder_restatement(golden, name):
    case = ec.make_encoder_case(name)
    agree(golden, "encoder/" + name, case, er.encoder_case(case), case["samples"])


def test_the_cases_cover_what_they_claim():
    kinds = {v[:4] for k, v in ec.CONV_KINDS.items() if k != "planted"}
    layers = {(k, s, cin, out) for _n, out, cin, k, s in ec.LAYERS}
    assert kinds == layers, "every (filter, stride, Cin, Cout) of the encoder and no other"
    assert {v[4] for v in ec.CONV_KINDS.values()} >= {"plain", "bn", "bn_relu", "bn_relu_res"}
    for B, H, W in ((3, 5, 7),):
        assert (B * H * W) % 64 and (B * ec.out_size(H, 2) * ec.out_size(W, 2)) % 64
    # the smallest images the reference takes under instance norm give 2 x 2 features; one pixel less gives planes of one element
    assert ec.out_size(9, 8) == 2 and ec.out_size(8, 8) == 1
    with pytest.raises(ValueError, match="more than 1 spatial element"):
        er.instance_norm(np.zeros((1, 2, 1, 1)))
    const = ec.make_norm_case("in_const")
    assert (er.norm_case(const)[:, 0] == 0.0).all()
    planted = ec.make_conv_case("planted_3x5x7")
    want = er.conv_case(planted)
    for ch, value in ec.PLANTED[0].items():
        assert (want[:, ch] == max(np.float32(value), 0.0)).all()
    for ch in ec.PLANTED[1]:
        assert (want[:, ch] == 0.0).all()


def test_the_raft_cases_are_the_minted_ones(golden):
    for name in ec.RAFT_CASES:
        case = ec.make_raft_case(name)
        assert ec.input_digest(case) == golden[f"raft/{name}/input_sha256"].tobytes().decode()
        assert tuple(case["state"]) == ec.RAFT_STATE_DICT_KEYS
        for o in ("flow_low", "flow_up"):
            assert golden[f"raft/{name}/{o}"].dtype == np.float32 and float(golden[f"raft/{name}/{o}_delta"]) > 0.0
    assert golden["state_dict_keys"].tolist() == list(ec.RAFT_STATE_DICT_KEYS) and len(ec.RAFT_STATE_DICT_KEYS) == 179
    assert os.path.getsize(er.GOLDEN) < 1000000


def test_the_module_has_the_reference_keys():
    """robust_cvd_amd.raft_ops.RAFT: the 179 keys in the reference's order, strict loading, DataParallel's prefix (no GPU touched)."""
    r = subprocess.run([sys.executable, "-m", "tests.raftenc_torch_child", "--keys"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "raft state dict keys ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
