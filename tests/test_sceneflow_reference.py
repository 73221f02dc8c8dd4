"""Scene-flow loss of flow pairs on the CPU: the numpy restatement (tests/sceneflow_reference.py) against the reference's committed
outputs (tests/golden/reference_py/sceneflow_golden.npz, minted by make_sceneflow_golden.py next to it from the reference's
SceneFlowLoss with torch autograd), the part of the gradient that flows through the static weight, the distance of the test
inputs from the sign kinks, and the exported symbols."""
import os

import numpy as np
import pytest

from tests import sceneflow_cases as sc
from tests import sceneflow_reference as sr

IDS = [sc.combo_key(c) for c in sc.COMBOS]


@pytest.fixture(scope="module")
def golden():
    return np.load(sr.GOLDEN)


def restatement(combo, **kw):
    case = sc.make_case(combo[0])
    return sr.scene_flow(**sc.case_kwargs(case), **sc.combo_kwargs(combo), **kw)


@pytest.mark.parametrize("combo", sc.COMBOS, ids=IDS)
def test_restatement_reproduces_the_committed_reference(golden, combo):
    """The same f64 arithmetic in another order: values to 1e-12, the gradient to 1e-11 x max |g|."""
    case, key = sc.make_case(combo[0]), sc.combo_key(combo)
    assert bytes(golden[f"{combo[0]}/digest"]).decode() == sc.digest(case)   # the fixture was minted from these inputs
    total, terms, g = restatement(combo, grad=True)
    ref_total, ref_terms, ref_g = float(golden[f"{key}/total"]), golden[f"{key}/terms"], golden[f"{key}/grad"]
    print(key, "total", abs(total - ref_total) / abs(ref_total), "grad", np.abs(g - ref_g).max() / np.abs(ref_g).max())
    assert abs(total - ref_total) <= 1e-12 * abs(ref_total)
    for q, name in enumerate(sr.TERMS):
        if combo[5][q] > 0:
            assert np.all(np.abs(terms[name] - ref_terms[:, q]) <= 1e-12 * np.abs(ref_terms[:, q])), name
        else:
            assert name not in terms and not ref_terms[:, q].any()
    assert np.abs(g - ref_g).max() <= 1e-11 * np.abs(ref_g).max()
    # what the f32 test leans on: the reference's own f32 noise, of the size seen when the fixture was minted
    assert 0 <= float(golden[f"{key}/delta_total"]) < 1e-6 and 0 < float(golden[f"{key}/delta_grad"]) < 1e-3


def test_restatement_reproduces_the_maps(golden):
    combo, key = sc.MAPS_COMBO, sc.combo_key(sc.MAPS_COMBO)
    maps = restatement(combo, maps=True)[-1]
    ref = golden[f"{key}/maps"]
    assert maps.shape == ref.shape and all(ref[k].any() for k in range(6))
    assert np.abs(maps - ref).max() <= 1e-12 * np.abs(ref).max()


def test_fixture_sees_the_gradient_through_the_static_weight(golden):
    """w = mask / |D_r| is a function of the depth and the reference does not detach it: the gradient that treats w as data
    differs from the fixture by far more than any tolerance of the kernel tests."""
    combo = sc.COMBOS[6]
    assert combo[5] == sc.STATIC_ONLY
    ref_g = golden[f"{sc.combo_key(combo)}/grad"]
    g = restatement(combo, grad=True, weight_is_data=True)[2]
    gap = np.abs(g - ref_g).max() / np.abs(ref_g).max()
    print("gradient without d w / d D: gap", gap)
    assert gap > 1e-2


def test_static_only_digests_and_structure():
    case = sc.make_case("odd")
    assert not case["nmasks"][2][1].any() and case["nmasks"][2][0].any()      # one neighbour mask all zero
    assert set(np.unique(case["masks"][0])) - {0.0, 1.0}                       # real weights, not only a mask
    assert sc.make_case("pair")["nbrs"] is None
    assert any(c[1] != c[2] for c in sc.COMBOS)                                # static and smooth distances differ somewhere


@pytest.mark.parametrize("name", list(sc.CASES))
def test_inputs_stay_away_from_the_sign_kinks(name):
    kinks = sr.check_kinks(sc.make_case(name))
    assert min(kinks) >= sr.KINK_DISTANCE, kinks


def test_scene_flow_symbols_are_exported():
    from robust_cvd_amd import api
    lib = api.load_library()
    for name in ("cvd_scene_flow_loss", "cvd_scene_flow_loss_device"):
        assert name in api.EXPORTED_SYMBOLS and hasattr(lib, name)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvd_hip.h")).read()
    assert "cvd_scene_flow_desc" in text and "CVD_ABI_REVISION 6" in text
    d = api.scene_flow_desc(1, 5, 3, 23, 37)
    assert d.struct_size == 88 | (api.ABI_REVISION << 32)
