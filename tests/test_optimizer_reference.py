"""The numpy restatement of the update rules and of the parameter regulariser (tests/optimizer_reference.py: what the GPU tests of
robust_cvd_amd/csrc/cvd_paramstep.h compare against) held to the reference's recorded run
(tests/golden/reference_py/optimizer_golden.npz); no GPU needed.  In float32 it must reproduce the reference's float32 results
within the bar of the GPU's f32 kernels, 8 x the reference's own f32-against-f64 spread (the fixture's, never below one rounding):
the restatement and the reference differ in operation order only (torch's lerp and addcdiv forms).  The maker script asserts the
float64 side (torch.optim.Adam in float64 within 1e-12)."""
import numpy as np
import pytest

from robust_cvd_amd import api
from tests import optimizer_cases as oc
from tests import optimizer_reference as orf


@pytest.fixture(scope="module")
def golden():
    g = np.load(orf.GOLDEN)
    case = oc.make_case()
    assert bytes(g["digest"]).decode() == oc.digest(case), "the fixture was minted for other inputs (or another PARAM_CHUNK)"
    assert np.array_equal(g["sample"], oc.sample_indices(case))
    return g


def test_the_yardstick_is_f32_rounding(golden):
    """The f32 bar is 8 x max |reference f32 - f64 restatement|.  A restatement that computed something else would widen that bar
    instead of failing a test, so the spread itself is held to f32 rounding: eight steps of a dozen roundings at 2^-24 of the
    array's scale stay below 1e-5 of it (the reference's RAdam and ParameterLoss and torch.optim.Adam, every element)."""
    keys = [k[:-len("/spread")] for k in golden.files if k.endswith("/spread") and k != "loss/spread"]
    assert len(keys) == 6 * len(oc.CONFIGS)
    for key in keys:
        ratio = float(golden[f"{key}/spread"]) / float(golden[f"{key}/scale"])
        assert ratio < 1e-5, (key, ratio)
    assert float(golden["loss/spread"]) / float(golden["loss/value"]) < 1e-5


def test_case_layout():
    case = oc.make_case()
    c = api.PARAM_CHUNK
    assert c >= 1024 and c & (c - 1) == 0
    assert case["counts"].tolist() == [0, 1, 3, 4, 5, 63, 64, 65, c - 1, c, c + 1, 2 * c + 7]
    rest = case["offsets"] % 4
    assert rest[oc.MISALIGNED] == 1 and not np.delete(rest, oc.MISALIGNED).any()
    ends = case["offsets"] + case["counts"]
    assert (case["offsets"][1:] >= ends[:-1]).all() and ends[-1] <= case["total"]
    used = case["used"]
    ties = (case["p"] == case["p0"])[used].mean()
    assert 0.33 <= ties <= 0.34, ties
    mag = np.abs(case["g"][:, used])
    assert mag.min() >= 0.99e-4 and mag.max() <= 1.0 and (mag < 1e-3).mean() > 0.2 and (mag > 0.1).mean() > 0.2
    for k in ("p", "p0", "g"):
        assert np.array_equal(case[k], case[k].astype(np.float32).astype(np.float64)), k


@pytest.mark.parametrize("config", list(oc.CONFIGS))
def test_f32_restatement_against_the_reference(golden, config):
    case = oc.make_case()
    got = orf.run(config, case, np.float32)
    for k, a in got.items():
        key = f"{config}/{k}"
        assert a.dtype == np.float32
        err = np.abs(a[golden["sample"]].astype(np.float64) - golden[key].astype(np.float64)).max()
        assert err < orf.bar(golden, key), (key, err, orf.bar(golden, key))


def test_regime_switch_at_step_6():
    """beta2 = 0.999: N_sma is 4.996 at step 5 and 5.994 at step 6."""
    rule = lambda step, sgd: orf.RULE[api.radam_record(step, 1e-2, degenerated_to_sgd=sgd).rule]
    assert [rule(k, True) for k in range(1, 9)] == ["radam_sgd"] * 5 + ["radam"] * 3
    assert [rule(k, False) for k in range(1, 9)] == ["moments"] * 5 + ["radam"] * 3
    n_sma = lambda t: (2 / (1 - 0.999) - 1) - 2 * t * 0.999 ** t / (1 - 0.999 ** t)
    assert abs(n_sma(5) - 4.996) < 1e-3 and abs(n_sma(6) - 5.994) < 1e-3
    # moments only: the parameters stay until the switch, and move at step 6 (the fixture: the reference does the same)
    case = oc.make_case()
    got = orf.run("radam-wd0.01-moments", case, np.float32)
    assert np.array_equal(got["p/5"], case["p"].astype(np.float32)) and not np.array_equal(got["p/6"], got["p/5"])
    # the degenerate rule is momentum SGD: no second moment in the step
    r = api.radam_record(1, 1e-2)
    assert r.step == 1e-2 / (1 - 0.9) and r.param_decay == 0.0 and r.denom_scale == 1.0
    a = api.adam_record(3, 1e-2, weight_decay=0.01)
    assert a.step == 1e-2 / (1 - 0.9 ** 3) and a.denom_scale == (1 - 0.999 ** 3) ** 0.5 and a.grad_decay == 0.01


def test_tie_subgradient(golden):
    case = oc.make_case()
    used = case["used"]
    for dtype in (np.float32, np.float64):
        g = orf.loss_grad(case, dtype)
        ties = (case["p"] == case["p0"]) & used
        k = np.dtype(dtype).type(oc.LAMBDA) * np.dtype(dtype).type(oc.GRAD_OUT)
        assert ties.sum() > used.sum() // 4 and not g[ties].any() and set(np.unique(g[used & ~ties]).tolist()) == {-float(k), float(k)}
    assert np.array_equal(orf.loss_grad(case, np.float32)[golden["sample"]], golden["loss/grad"])
    value = float(golden["loss/value"])
    assert abs(orf.loss(case, np.float64) - value) <= 1e-12 * value
    assert abs(orf.loss(case, np.float32) - value) < 8 * max(float(golden["loss/spread"]), orf.EPS32 * value)
