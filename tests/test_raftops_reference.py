"""CPU checks of the RAFT operator fixture (tests/golden/reference_py/raftops_golden.npz, minted from the reference's CorrBlock and
RAFT.upsample_flow by make_raftops_golden.py): the float64 restatement the GPU tests measure against (tests/raftops_reference.py)
reproduces the reference's stored f32 outputs within the reference's own recorded error, the generators still build the inputs the
fixture was minted from, and, where the reference checkout is mounted, it still gives the stored outputs exactly."""
import numpy as np
import pytest

from tests import raftops_cases as rc
from tests import raftops_reference as rr


@pytest.fixture(scope="module")
def golden():
    return np.load(rr.GOLDEN)


@pytest.fixture(scope="module")
def corr_cases():
    return {name: rc.make_corr_case(name) for name in rc.CORR}


@pytest.fixture(scope="module")
def restated(corr_cases):
    out = {}
    for name, case in corr_cases.items():
        pyr = rr.pyramid(case["raw"], case["dim"], case["levels"])
        out[name] = (pyr, rr.lookup(pyr, case["coords"], case["r"]))
    return out


@pytest.mark.parametrize("name", list(rc.CORR) + list(rc.UPSAMPLE))
def test_inputs_are_the_minted_ones(golden, name):
    case = rc.make_corr_case(name) if name in rc.CORR else rc.make_upsample_case(name)
    assert rc.input_digest(case) == golden[name + "/input_sha256"].tobytes().decode()


@pytest.mark.parametrize("name", list(rc.CORR))
def test_case_shapes(corr_cases, golden, name):
    case = corr_cases[name]
    B, h, w, dim, levels, r = rc.CORR[name]
    q = golden[name + "/queries"]
    assert np.array_equal(q, case["queries"])
    assert len(q) == min(B * h * w, rc.SAMPLED_QUERIES) and set(range(13)) <= set(q.tolist()) and B * h * w - 1 in q
    assert golden[name + "/lookup"].shape == (len(q), levels * (2 * r + 1) ** 2)
    for l in range(1, levels):
        assert golden[f"{name}/pyr{l}"].shape == (len(q), h >> l, w >> l)
    assert min(h >> (levels - 1), w >> (levels - 1)) >= 2


@pytest.mark.parametrize("name", list(rc.CORR))
def test_restatement_reproduces_the_reference_pyramid(corr_cases, restated, golden, name):
    case = corr_cases[name]
    pyr = restated[name][0]
    # level 0: the f64 quotient rounds to the f32 quotient (one division, correctly rounded in both)
    assert np.array_equal(pyr[0].astype(np.float32), rr.level0_f32(case["raw"], case["dim"]))
    delta = float(golden[name + "/delta_pyr"])
    for l in range(1, case["levels"]):
        err = np.abs(golden[f"{name}/pyr{l}"] - pyr[l][case["queries"]]).max()
        assert err <= delta, (l, err, delta)
    assert max(np.abs(a).max() for a in pyr[1:]) == float(golden[name + "/scale_pyr"])


@pytest.mark.parametrize("name", list(rc.CORR))
def test_restatement_reproduces_the_reference_lookup(corr_cases, restated, golden, name):
    case = corr_cases[name]
    look = restated[name][1]
    stored = golden[name + "/lookup"]
    err = np.abs(stored - rc.query_view(case, look)).max()
    assert err <= float(golden[name + "/delta_lookup"]), (err, float(golden[name + "/delta_lookup"]))
    assert np.abs(look).max() == float(golden[name + "/scale_lookup"])
    # the planted outside and huge coordinates: exact zeros in the reference and in the restatement
    where = np.searchsorted(case["queries"], rc.ZERO_CELLS)
    assert not stored[where].any() and not rc.query_view(case, look)[where].any()
    # ... and the cells next to them are not (the planting hit the cells it names)
    assert stored[np.searchsorted(case["queries"], [0, 1, 2, 3, 4, 5, 6])].any(axis=1).all()


def test_the_first_window_index_moves_x(restated, corr_cases):
    """Channel a n + b of level 0 at an integer position is the map's texel (x + a - r, y + b - r)."""
    case = corr_cases["square16"]
    pyr, look = restated["square16"]
    r, n = case["r"], 2 * case["r"] + 1
    x, y = case["coords"][0, :, 0, 0]      # cell 0: planted (3, 5)
    assert (x, y) == (3.0, 5.0)
    for a, b in ((0, 0), (n - 1, 0), (2, 7), (r, r)):
        tx, ty = int(x) + a - r, int(y) + b - r
        want = pyr[0][0, ty, tx] if 0 <= tx < case["w"] and 0 <= ty < case["h"] else 0.0
        assert look[0, a * n + b, 0, 0] == want, (a, b)


@pytest.mark.parametrize("name", list(rc.UPSAMPLE))
def test_restatement_reproduces_the_reference_upsampling(golden, name):
    case = rc.make_upsample_case(name)
    up = rr.upsample(case["flow"], case["mask"])
    assert np.isfinite(up).all()
    assert np.abs(golden[name + "/out"] - up).max() <= float(golden[name + "/delta"])
    assert np.abs(up).max() == float(golden[name + "/scale"])


def test_live_reference_gives_the_stored_outputs(golden, corr_cases):
    ref = rr.load_reference()
    if ref is None:
        pytest.skip("the reference checkout (or torch) is not available here")
    for name, case in corr_cases.items():
        pyr32, look32 = rr.reference_outputs(ref, case)
        assert np.array_equal(pyr32[0], rr.level0_f32(case["raw"], case["dim"]))
        for l in range(1, case["levels"]):
            assert np.array_equal(pyr32[l][case["queries"]], golden[f"{name}/pyr{l}"])
        assert np.array_equal(rc.query_view(case, look32), golden[name + "/lookup"])
    for name in rc.UPSAMPLE:
        assert np.array_equal(rr.reference_upsample(ref, rc.make_upsample_case(name)), golden[name + "/out"])
