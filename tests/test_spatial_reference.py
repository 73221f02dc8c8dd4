"""The numpy restatement of the spatial losses (tests/spatial_reference.py) against the reference's recorded outputs
(tests/golden/reference_py/spatial_golden.npz, minted by make_spatial_golden.py from the reference's own modules), the conditions
on the seeded cases, and the restatement's gradient against finite differences.  No GPU, no reference checkout."""
import numpy as np
import pytest

from tests import spatial_cases as sc
from tests import spatial_reference as sr

IDS = [sc.combo_key(c) for c in sc.COMBOS]


@pytest.fixture(scope="module")
def golden():
    return np.load(sr.GOLDEN)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_cases_are_the_recorded_ones_and_hold_their_conditions(golden, name):
    case = sc.make_case(name)
    assert bytes(golden[f"{name}/digest"]).decode() == sc.digest(case)
    assert case["depth"].shape == (case["B"] * case["N"], case["H"], case["W"]) and case["depth"].min() > 0.5
    assert 0.0 <= case["image"].min() and case["image"].max() <= 1.0
    for k in ("depth", "depth_orig", "image"):
        assert np.array_equal(case[k], case[k].astype(np.float32).astype(np.float64)), k
    rel = np.abs(case["depth"] / case["depth_orig"] - 1.0)
    assert 0.005 < rel.mean() < 0.05 and rel.max() < 0.08      # a few percent apart
    kd, kD, gap, share = sr.check_conditions(case, sc.THRESHOLDS)
    assert kd >= sr.KINK_DISTANCE and kD >= sr.KINK_DISTANCE, (kd, kD)
    assert gap >= sr.THRESHOLD_DISTANCE, gap
    if name != "tiny":
        for tau, v in share.items():
            assert sr.MASK_SHARE[0] <= v <= sr.MASK_SHARE[1], (tau, v)


def test_combinations_cover_the_issue():
    assert {c[0] for c in sc.COMBOS} == {"tiny", "odd", "aligned", "six"}
    for case in sc.CASES:
        mine = [c for c in sc.COMBOS if c[0] == case]
        assert any(c[1] > 0 and c[3] > 0 for c in mine) and any(c[1] > 0 and c[3] == 0 for c in mine)
        assert any(c[1] == 0 and c[3] > 0 for c in mine) and any((c[2], c[4]) == (0.25, 1.2) for c in mine)
    assert sc.CASES["odd"]["W"] % 4 and sc.CASES["aligned"]["W"] % 4 == 0 and sc.CASES["six"]["N"] == 6


@pytest.mark.parametrize("combo", sc.COMBOS, ids=IDS)
def test_restatement_reproduces_the_reference(golden, combo):
    key, case = sc.combo_key(combo), sc.make_case(combo[0])
    total, smooth, contrast, g = sr.spatial(**sc.case_kwargs(case), **sc.combo_kwargs(combo), grad=True)
    ref_total, ref_g = float(golden[f"{key}/total"]), golden[f"{key}/grad"]
    assert abs(total - ref_total) <= 1e-12 * abs(ref_total)
    assert np.all(np.abs(smooth - golden[f"{key}/smooth"]) <= 1e-12 * np.abs(golden[f"{key}/smooth"]))
    assert abs(contrast - float(golden[f"{key}/contrast"])) <= 1e-12 * abs(float(golden[f"{key}/contrast"]))
    assert (smooth > 0).all() == (combo[1] > 0) and (contrast > 0) == (combo[3] > 0)
    assert np.abs(g - ref_g).max() <= 1e-12 * np.abs(ref_g).max()
    assert float(golden[f"{key}/delta_total"]) < 1e-5 and float(golden[f"{key}/delta_grad"]) < 1e-5


@pytest.mark.parametrize("setting", ["both", "smooth", "contrast", "second"])
def test_restatement_gradient_against_finite_differences(setting):
    """Central differences on a dozen pixels of `odd`: the four corners, last-row and last-column pixels, interior pixels.  The
    step 1e-4 stays inside the smooth piece (the nearest kink of `odd` is 9e-4 away in disparity, 3e-3 in depth).  Bar 1e-6 x
    max |g|: the truncation error is h^2 / 6 times a third derivative a few times the first, 1e-8 relative; the rounding of the
    two totals (at most 166, sums of 1e4 terms) is about 10 x 2^-52 x 166 / h = 4e-9 against gradients of 0.1, and 7e-13
    against 2e-5 for the smoothness term alone (total 0.03)."""
    combo = ("odd",) + sc.SETTINGS[setting]
    case = sc.make_case("odd")
    H, W, F = case["H"], case["W"], case["F"]
    kw = dict(sc.case_kwargs(case), **sc.combo_kwargs(combo))
    g = sr.spatial(**kw, grad=True)[3]
    pixels = [(0, 0, 0), (1, 0, W - 1), (2, H - 1, 0), (3, H - 1, W - 1), (4, H - 1, 11), (5, 7, W - 1), (0, H - 1, W - 2),
              (1, 0, 5), (2, 9, 0), (3, 11, 17), (4, 12, 18), (5, 3, 35)]
    assert len(pixels) >= 12 and all(f < F for f, _y, _x in pixels)
    h = 1e-4
    for f, y, x in pixels:
        vals = []
        for sgn in (1.0, -1.0):
            D = np.array(kw["depth"])
            D[f, y, x] += sgn * h
            vals.append(sr.spatial(**dict(kw, depth=D))[0])
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - g[f, y, x]) <= 1e-6 * np.abs(g).max(), (f, y, x, fd, g[f, y, x])


def test_joint_record_is_complete(golden):
    from tests import sceneflow_cases as sfc
    case = sfc.make_case(sc.JOINT_CASE)
    assert bytes(golden["joint/digest"]).decode() == sfc.digest(case)
    names = {k.split("/", 2)[2] for k in golden.files if k.startswith("joint/batch/")}
    assert names == {"parameter_loss", "reproj", "disp", "depth ratio", "static", "smooth_reproj", "smooth_disparity",
                     "smooth_depth_ratio", "disparity_smooth"}
    # the total is the sum of the terms, up to the float32 tensor the reference sums it in
    terms = [float(golden["joint/batch/parameter_loss"].sum()), float(golden["joint/contrast"])]
    terms += [float(golden[f"joint/batch/{k}"].mean()) for k in names - {"parameter_loss"}]
    assert abs(float(golden["joint/total"]) - sum(terms)) <= 8 * 2.0 ** -23 * sum(abs(v) for v in terms)
    extra = sc.joint_inputs(case)
    lam = sc.JOINT_OPTIONS["lambda_parameter"]
    for i, (p, p0) in enumerate(zip(extra["parameters"], extra["parameters_init"])):
        assert np.array_equal(golden[f"joint/parameter_grad/{i}"], lam * np.sign(p - p0))
    # the spatial part of the record: the restatement on the joint inputs
    _total, smooth, contrast = sr.spatial(case["depth"], extra["depth_orig"], extra["image"], frames_per_sample=6,
                                          lambda_disparity_smooth=sc.JOINT_OPTIONS["lambda_disparity_smooth"],
                                          sigma_color_grad=sc.JOINT_OPTIONS["sigma_color_grad"],
                                          lambda_contrast_loss=sc.JOINT_OPTIONS["lambda_contrast_loss"],
                                          contrast_thresh=sc.JOINT_OPTIONS["lambda_contrast_thresh"])
    assert np.all(np.abs(smooth - golden["joint/batch/disparity_smooth"]) <= 1e-12 * smooth)
    assert abs(contrast - float(golden["joint/contrast"])) <= 1e-12 * contrast
