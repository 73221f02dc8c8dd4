"""Flow consistency masks on the CPU: the numpy restatement (tests/flowmask_reference.py) against the reference's committed
outputs (tests/golden/reference_py/flowmask_golden.npz, minted by make_flowmask_golden.py next to it from the reference's
utils/consistency.py), live against the reference where it is mounted, and known answers of the definition."""
import os

import numpy as np
import pytest

from robust_cvd_amd import dataset_io
from tests import flowmask_cases as fc
from tests import flowmask_reference as fr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "flowmask_golden.npz")


def golden_case(g, name):
    """(reference masks [U, 2, H, W] bool, undecided [U, 2, H, W] bool, err_pairs, errors [n, 2, H, W, 2] f32, delta, delta_rel)."""
    shape = tuple(g[name + "/shape"].tolist())
    n = int(np.prod(shape))
    masks = np.unpackbits(g[name + "/mask_bits"])[:n].reshape(shape).astype(bool)
    und = np.unpackbits(g[name + "/undecided_bits"])[:n].reshape(shape).astype(bool)
    src = g[name + "/errors_case"].tobytes().decode() if name + "/errors_case" in g.files else name
    return masks, und, g[name + "/err_pairs"], g[src + "/errors"], float(g[name + "/delta"]), float(g[name + "/delta_rel"])


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_restatement_reproduces_the_committed_reference_masks(name):
    g = np.load(GOLDEN)
    case = fc.make_case(name)
    assert fc.input_digest(case).encode() == g[name + "/input_sha256"].tobytes(), "the seeded case drifted from the minted one"
    masks, und, ep, err_ref, delta, delta_rel = golden_case(g, name)
    # the cap on the band, on the stored arrays: at most 0.1 % of a case's pixels are undecided, and the stored flags are
    # the band of the stored errors
    assert und.mean() <= fr.MAX_UNDECIDED and und.mean() == float(g[name + "/undecided_share"])
    C = case["color"].shape[-1]
    assert np.array_equal(fr.undecided(err_ref, delta, case["flow_thresh"], case["color_thresh"], C), und[ep])
    mab, mba, kept, err = fr.batch(case["color"], case["pairs"], case["flow_ab"], case["flow_ba"], case["flow_thresh"],
                                   case["color_thresh"])
    mine = np.stack([mab, mba], axis=1) > 0
    print(f"{name}: delta {delta:.3e} delta_rel {delta_rel:.3e} undecided {int(und.sum())} of {und.size}, kept "
          f"{100 * masks.mean():.1f} %, differing decided pixels {int(((mine != masks) & ~und).sum())}")
    assert 0.2 < masks.mean() < 0.8            # both outcomes are well represented
    assert np.array_equal(mine[~und], masks[~und])
    assert fr.errors_close(err[ep], err_ref, delta, delta_rel).all()
    assert np.array_equal(kept, np.stack([(mab > 0).sum((1, 2)), (mba > 0).sum((1, 2))], 1))


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_restatement_against_the_live_reference(name):
    cons = fr.load_reference_consistency()
    if cons is None:
        pytest.skip("the reference (utils/consistency.py) or torch is not on this machine")
    g = np.load(GOLDEN)
    case = fc.make_case(name)
    masks, und, _ep, _err, delta, delta_rel = golden_case(g, name)
    color, pairs = case["color"], case["pairs"]
    mab, mba, _kept, err = fr.batch(color, pairs, case["flow_ab"], case["flow_ba"], case["flow_thresh"], case["color_thresh"])
    for p, (a, b) in enumerate(pairs.tolist()):
        live, live_err = fr.reference_pair(cons, case["flow_ab"][p], case["flow_ba"][p], color[a], color[b],
                                           case["flow_thresh"], case["color_thresh"])
        assert np.array_equal(live[~und[p]], masks[p][~und[p]])  # the committed file is what the reference computes
        mine = np.stack([mab[p], mba[p]]) > 0
        assert np.array_equal(mine[~und[p]], live[~und[p]])
        assert fr.errors_close(err[p], live_err, delta, delta_rel).all()


def _pair(H, W, C=3):
    z = np.zeros((H, W, 2), np.float32)
    return z.copy(), z.copy(), np.full((H, W, C), 0.25, np.float32), np.full((H, W, C), 0.25, np.float32)


def test_constant_colour_and_zero_flows_keep_every_pixel():
    fab, fba, ca, cb = _pair(7, 9)
    mab, mba = fr.pair_masks(fab, fba, ca, cb)
    assert mab.dtype == np.uint8 and (mab == 255).all() and (mba == 255).all()


def test_one_hot_target_shows_the_half_pixel_shift():
    """Zero flow samples the target at (x - 0.5, y - 0.5): a one-hot target image at (5, 3) is seen with weight 1/4 by the four
    pixels (5, 3), (6, 3), (5, 4), (6, 4) -- not with weight 1 by (5, 3) alone, as a sampler at x + flow would."""
    H, W = 8, 16  # (powers of two: gx, gy are exact in f32, so the weights are exactly 1/4)
    fab, fba, ca, cb = _pair(H, W, 1)
    ca[:], cb[:] = 0.0, 0.0
    cb[3, 5, 0] = 4.0
    _inb, _ef, ec = fr.direction_errors(fab, fba, ca, cb)
    expect = np.zeros((H, W))
    expect[3:5, 5:7] = 1.0  # (0 - 4 / 4)^2
    assert np.array_equal(ec, expect)
    mab = fr.direction_mask(fab, fba, ca, cb, 1.0, 1.0)       # ec < 1 fails exactly there
    assert np.array_equal(mab == 0, expect == 1.0)
    # the border rule: pixel (0, 0) samples (-0.5, -0.5), clamped to texel (0, 0) with weight 1
    cb[:] = 0.0
    cb[0, 0, 0] = 4.0
    _inb, _ef, ec = fr.direction_errors(fab, fba, ca, cb)
    assert ec[0, 0] == 16.0 and ec[0, 1] == 4.0 and ec[1, 1] == 1.0


def test_flow_error_just_above_the_threshold_is_rejected():
    fab, fba, ca, cb = _pair(6, 12)
    fab[..., 0] = 2.0
    fba[..., 0] = -1.0                       # |Fab + S(Fba)| = 1 exactly: not < 1
    mab = fr.direction_mask(fab, fba, ca, cb)
    assert (mab[:, :10] == 0).all()
    fba[..., 0] = np.nextafter(np.float32(-1.0), np.float32(-2.0))  # |.| just below 1
    mab = fr.direction_mask(fab, fba, ca, cb)
    assert (mab[:, :10] == 255).all() and (mab[:, 10:] == 0).all()   # (the last two columns leave the image)
    fba[..., 0] = np.nextafter(np.float32(-1.0), np.float32(0.0))   # 1 + 6e-8: just above
    assert (fr.direction_mask(fab, fba, ca, cb)[:, :10] == 0).all()


def test_out_of_bounds_by_one_ulp_is_rejected():
    H, W = 5, 8
    fab, fba, ca, cb = _pair(H, W)
    fab[2, 3, 0] = 4.0                                              # x + flow = W - 1: inside
    fab[2, 4, 0] = np.nextafter(np.float32(3.0), np.float32(4.0))   # one f32 ulp beyond W - 1
    fab[1, 0, 0] = -np.finfo(np.float32).tiny                       # just below 0 (exact in f64)
    fab[4, 1, 1] = np.finfo(np.float32).tiny                        # H - 1 + 1e-38 IS H - 1 in f64, the sum's precision: inside
    mab = fr.direction_mask(fab, fba, ca, cb, flow_thresh=100.0)
    assert mab[2, 3] == 255 and mab[2, 4] == 0 and mab[1, 0] == 0 and mab[4, 1] == 255
    assert (mab == 0).sum() == 2


def test_nan_is_rejected():
    fab, fba, ca, cb = _pair(6, 6)
    fab[1, 1, 0] = np.nan      # own flow
    fba[3, 3, 1] = np.nan      # a tap of pixels (3, 3), (4, 3), (3, 4), (4, 4)
    cb[0, 5, 2] = np.nan       # a tap of pixels (5, 0) and (5, 1) (x, y)
    mab = fr.direction_mask(fab, fba, ca, cb)
    bad = np.zeros((6, 6), bool)
    bad[1, 1] = True
    bad[3:5, 3:5] = True
    bad[0:2, 5] = True
    assert np.array_equal(mab == 0, bad)


def test_read_raw_image_inverts_write_raw_image(tmp_path):
    rng = np.random.default_rng(2)
    for shape in ((5, 7), (5, 7, 2), (4, 6, 3)):
        img = rng.normal(size=shape).astype(np.float32)
        path = str(tmp_path / "img.raw")
        dataset_io.write_raw_image(path, img)
        back = dataset_io.read_raw_image(path)
        assert back.dtype == np.float32 and back.shape == shape and np.array_equal(back, img)
    with open(path, "r+b") as f:
        f.truncate(40)
    with pytest.raises(ValueError, match="img.raw"):
        dataset_io.read_raw_image(path)


def test_pair_stats_from_png_files(tmp_path):
    """compute_flow_pair_stats without a GPU: ratios read back from PNG masks, rows in the order of frame_pairs, a pair and its
    reverse once, an existing file returned untouched."""
    import json
    from robust_cvd_amd import flow_masks
    H, W = 6, 10
    rng = np.random.default_rng(4)
    pairs = np.array([[0, 1], [1, 0], [0, 2], [2, 0]], np.int32)
    masks = np.where(rng.uniform(size=(4, H, W)) < 0.6, 255, 0).astype(np.uint8)
    base = str(tmp_path)
    dataset_io.write_flow_inputs(base, pairs, np.zeros((4, H, W, 2), np.float32), masks, np.zeros((3, H, W, 3), np.float32))
    path = flow_masks.compute_flow_pair_stats(base, [(0, 2), (0, 1), (1, 0), (2, 0)])
    assert path == os.path.join(base, "flow_list.json")
    rows = json.load(open(path))
    cnt = (masks > 0).sum(axis=(1, 2))
    r01, r02 = min(cnt[0], cnt[1]) / (H * W), min(cnt[2], cnt[3]) / (H * W)
    assert rows == [["frame0", "frame1", "mask_ratio"], [0, 2, r02], [2, 0, r02], [0, 1, r01], [1, 0, r01]]
    before = open(path, "rb").read()
    assert flow_masks.compute_flow_pair_stats(base, [(0, 1)]) == path and open(path, "rb").read() == before
