"""Consistency loss of flow pairs on the CPU: the numpy restatement (tests/consistency_reference.py) against the reference's
committed outputs (tests/golden/reference_py/consistency_golden.npz, minted by make_consistency_golden.py next to it from the
reference's ConsistencyLoss with torch autograd), its gradient against central differences of its own forward, the distance of
the test inputs from the sign kinks, live against the reference where it is mounted, and the exported symbols."""
import os

import numpy as np
import pytest

from tests import consistency_cases as cc
from tests import consistency_reference as cr

IDS = [cc.combo_key(c) for c in cc.COMBOS]


@pytest.fixture(scope="module")
def golden():
    return np.load(cr.GOLDEN)


def restatement(combo, **kw):
    case = cc.make_case(combo[0])
    return cr.consistency(*cc.case_args(case), distance=combo[1], scale=combo[2], alpha=combo[3], lambdas=combo[4], **kw)


@pytest.mark.parametrize("combo", cc.COMBOS, ids=IDS)
def test_restatement_reproduces_the_committed_reference(golden, combo):
    """f64 against reference-held values: 1e-10 x their size, the gradient to 1e-9 x max |g|."""
    case, key = cc.make_case(combo[0]), cc.combo_key(combo)
    assert bytes(golden[f"{combo[0]}/digest"]).decode() == cc.digest(case)   # the fixture was minted from these inputs
    total, terms, g = restatement(combo, grad=True)
    ref_terms = golden[f"{key}/terms"]
    assert abs(total - float(golden[f"{key}/total"])) <= 1e-10 * abs(float(golden[f"{key}/total"]))
    for q, name in enumerate(cr.TERMS):
        if combo[4][q] > 0:
            assert np.all(np.abs(terms[name] - ref_terms[:, q]) <= 1e-10 * np.abs(ref_terms[:, q])), name
        else:
            assert name not in terms and not ref_terms[:, q].any()
    ref_g = golden[f"{key}/grad"]
    assert np.abs(g - ref_g).max() <= 1e-9 * np.abs(ref_g).max()
    # what the f32 test leans on: the reference's own f32 noise, of the size seen when the fixture was minted
    assert 0 <= float(golden[f"{key}/delta_total"]) < 1e-6 and 0 < float(golden[f"{key}/delta_grad"]) < 1e-3


@pytest.mark.parametrize("combo", [cc.COMBOS[7], cc.COMBOS[4], cc.COMBOS[10]], ids=[IDS[7], IDS[4], IDS[10]])
def test_restatement_gradient_against_central_differences(combo):
    """Central differences (step 1e-6, far inside the 1e-5 kink distance times the errors' depth derivatives) of the restatement's
    own forward at 16 seeded depth entries per frame kind.  Truncation is O(h^2); rounding is eps |total| / h ~ 1e-16 x 50 / 1e-6 =
    5e-9 absolute, against gradients of 1e-3 .. 1e-1: the bar is 1e-5 x max |g|."""
    case = cc.make_case(combo[0])
    args = list(cc.case_args(case))
    kw = dict(distance=combo[1], scale=combo[2], alpha=combo[3], lambdas=combo[4])
    _t, _terms, g = cr.consistency(*args, grad=True, **kw)
    rng = np.random.default_rng(77)
    h = 1e-6
    worst = 0.0
    for _ in range(16):
        idx = (rng.integers(case["F"]), rng.integers(case["H"]), rng.integers(case["W"]))
        vals = []
        for sgn in (1.0, -1.0):
            d = args[0].copy()
            d[idx] += sgn * h
            vals.append(cr.consistency(d, *args[1:], **kw)[0])
        worst = max(worst, abs((vals[0] - vals[1]) / (2 * h) - g[idx]))
    assert worst <= 1e-5 * np.abs(g).max(), (worst, np.abs(g).max())


@pytest.mark.parametrize("name", list(cc.CASES))
def test_inputs_stay_away_from_the_sign_kinks(name):
    """Every weighted sample's e_rep, |e_dsp| and |e_rat| / lambda_ratio are >= 1e-5: about a hundred f32 roundings."""
    kinks = cr.check_kinks(cc.make_case(name))
    assert min(kinks) >= cr.KINK_DISTANCE, kinks


def test_masked_direction_and_sides():
    case = cc.make_case("odd")
    assert not case["weight_ba"][1].any() and case["weight_ab"][1].any()
    assert set(np.unique(case["weight_ab"])) - {0.0, 1.0}     # real weights, not only a mask


@pytest.mark.parametrize("combo", [cc.COMBOS[0], cc.COMBOS[6], cc.COMBOS[11]], ids=[IDS[0], IDS[6], IDS[11]])
def test_fixture_against_the_live_reference(golden, combo):
    try:
        import torch  # noqa: F401
        total, terms, g = cr.reference_run(cc.make_case(combo[0]), *combo[1:], "float64")
    except ImportError:
        pytest.skip("the reference (loss/consistency_loss.py) or torch is not on this machine")
    key = cc.combo_key(combo)
    # (not bit for bit: torch's CPU reductions split their sums by the number of threads)
    assert abs(total - float(golden[f"{key}/total"])) <= 1e-12 * abs(total)
    assert np.abs(g - golden[f"{key}/grad"]).max() <= 1e-12 * np.abs(g).max()
    for q, name in enumerate(cr.TERMS):
        if name in terms:
            assert np.all(np.abs(terms[name] - golden[f"{key}/terms"][:, q]) <= 1e-12 * np.abs(terms[name]))


def test_consistency_symbols_are_exported():
    from robust_cvd_amd import api
    lib = api.load_library()
    for name in ("cvd_consistency_loss", "cvd_consistency_loss_device"):
        assert name in api.EXPORTED_SYMBOLS and hasattr(lib, name)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvd_hip.h")).read()
    assert "cvd_consistency_desc" in text and "CVD_ABI_REVISION 6" in text
    d = api.consistency_desc(1, 4, 3, 23, 37)
    assert d.struct_size == 80 | (api.ABI_REVISION << 32)
