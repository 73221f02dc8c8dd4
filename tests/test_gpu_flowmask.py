"""GPU parity of the flow consistency masks (robust_cvd_amd/csrc/cvd_flowmask.h; Flow.compute_flow_masks, reference
flow.py:180-209 + utils/consistency.py:8-67) against the reference's committed outputs
(tests/golden/reference_py/flowmask_golden.npz), through Solver.flow_consistency_masks and through the file-level drop-ins
robust_cvd_amd.flow_masks.compute_flow_masks / compute_flow_pair_stats.

Tolerance: a thresholded bit cannot be compared between two f32 implementations that round in different
orders, so the pixels whose REFERENCE error lies within 8 delta of a threshold are left out, delta = max |e_ref32 - e_f64| as
measured when the golden file was minted (never from this kernel); at most 0.1 % of a case's pixels may be undecided.  Every
other pixel's mask must equal the reference's, and the error maps must agree within 8 delta absolutely below 10 and within
8 delta_rel relatively above."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

from robust_cvd_amd import build as _b
from robust_cvd_amd import dataset_io, flow_masks, synth
from tests import flowmask_cases as fc
from tests import flowmask_reference as fr
from tests.test_flowmask_reference import GOLDEN, golden_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from robust_cvd_amd.api import Solver
    return Solver(0)


def run(solver, case, **kw):
    return solver.flow_consistency_masks(case["color"], case["pairs"], case["flow_ab"], case["flow_ba"], case["flow_thresh"],
                                         case["color_thresh"], **kw)


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_masks_and_errors_match_the_committed_reference_outputs(solver, name):
    g = np.load(GOLDEN)
    case = fc.make_case(name)
    assert fc.input_digest(case).encode() == g[name + "/input_sha256"].tobytes(), "the seeded case drifted from the minted one"
    masks, und, ep, err_ref, delta, delta_rel = golden_case(g, name)
    assert und.mean() <= fr.MAX_UNDECIDED
    mab, mba, kept, err = run(solver, case, return_errors=True)
    assert set(np.unique(mab)) <= {0, 255} and set(np.unique(mba)) <= {0, 255}
    mine = np.stack([mab, mba], axis=1) > 0
    a, b = err[ep].astype(np.float64), err_ref.astype(np.float64)
    fin = np.isfinite(b)
    small = fin & (b < fr.SMALL)
    big = fin & ~small
    with np.errstate(invalid="ignore"):
        d_abs = np.abs(a - b)[small].max() if small.any() else 0.0
        d_rel = (np.abs(a - b)[big] / np.abs(b[big])).max() if big.any() else 0.0
    print(f"{name}: delta {delta:.3e} delta_rel {delta_rel:.3e}; kernel vs reference: max abs {d_abs:.3e} (bound {8 * delta:.3e}), "
          f"max rel {d_rel:.3e} (bound {8 * delta_rel:.3e}); undecided {int(und.sum())} of {und.size}; differing decided pixels "
          f"{int(((mine != masks) & ~und).sum())}, differing undecided pixels {int(((mine != masks) & und).sum())}")
    assert np.array_equal(mine[~und], masks[~und])
    assert fr.errors_close(err[ep], err_ref, delta, delta_rel).all()
    assert np.array_equal(kept, np.stack([(mab > 0).sum((1, 2)), (mba > 0).sum((1, 2))], 1))
    # the f64 restatement agrees on the same terms
    rab, rba, _k, _e = fr.batch(case["color"], case["pairs"], case["flow_ab"], case["flow_ba"], case["flow_thresh"],
                                case["color_thresh"])
    assert np.array_equal(mine[~und], (np.stack([rab, rba], axis=1) > 0)[~und])


@pytest.mark.parametrize("name", ["w96_t1_1", "w50_t1_1", "w96_c1"])
def test_batched_call_equals_per_pair_calls_and_repeats_bit_for_bit(solver, name):
    case = fc.make_case(name)
    mab, mba, kept, err = run(solver, case, return_errors=True)
    again = run(solver, case, return_errors=True)
    for x, y in zip((mab, mba, kept, err), again):
        assert x.tobytes() == y.tobytes()
    plain = run(solver, case)                      # errors = NULL
    assert len(plain) == 3 and plain[0].tobytes() == mab.tobytes() and plain[1].tobytes() == mba.tobytes()
    assert np.array_equal(plain[2], kept)
    for p, (a, b) in enumerate(case["pairs"].tolist()):
        one = solver.flow_consistency_masks(case["color"][[a, b]], [[0, 1]], case["flow_ab"][p:p + 1], case["flow_ba"][p:p + 1],
                                            case["flow_thresh"], case["color_thresh"], return_errors=True)
        assert one[0][0].tobytes() == mab[p].tobytes() and one[1][0].tobytes() == mba[p].tobytes()
        assert np.array_equal(one[2][0], kept[p]) and one[3][0].tobytes() == err[p].tobytes()
    # a pair given in the other order is the same pair with the directions swapped
    p = len(case["pairs"]) - 1
    a, b = case["pairs"][p].tolist()
    swapped = solver.flow_consistency_masks(case["color"], [[b, a]], case["flow_ba"][p:p + 1], case["flow_ab"][p:p + 1],
                                            case["flow_thresh"], case["color_thresh"], return_errors=True)
    assert swapped[0][0].tobytes() == mba[p].tobytes() and swapped[1][0].tobytes() == mab[p].tobytes()
    assert swapped[3][0, 0].tobytes() == err[p, 1].tobytes() and swapped[2][0].tolist() == kept[p][::-1].tolist()


def test_both_thread_to_pixel_maps_produce_the_same_bits(solver):
    case = fc.make_case("w96_t1_1")              # width 96: the product call takes four pixels per thread
    auto = run(solver, case, return_errors=True)
    for pix in (1, 4):
        forced = run(solver, case, return_errors=True, pixels_per_thread=pix)
        for x, y in zip(auto, forced):
            assert x.tobytes() == y.tobytes(), pix
    odd = fc.make_case("w50_t1_1")               # width 50: one pixel per thread; the wide map is refused
    with pytest.raises(RuntimeError, match=r"multiple of 4 \(got 50\)"):
        run(solver, odd, pixels_per_thread=4)
    with pytest.raises(RuntimeError, match=r"pixels_per_thread must be 0, 1 or 4 \(got 2\)"):
        run(solver, case, pixels_per_thread=2)


def test_argument_checks(solver):
    case = fc.make_case("w50_t1_1")
    col, pairs, fab, fba = case["color"], case["pairs"], case["flow_ab"], case["flow_ba"]
    F, H, W, ch = col.shape
    P = len(pairs)
    mab, mba = np.zeros((P, H, W), np.uint8), np.zeros((P, H, W), np.uint8)
    fn = solver._fn("flow_consistency_masks")

    def call(**kw):
        a = dict(num_frames=F, height=H, width=W, channels=ch, color=col, num_pairs=P, pair_frames=pairs, flow_ab=fab,
                 flow_ba=fba, flow_thresh=1.0, color_thresh=1.0, mask_ab=mab, mask_ba=mba)
        a.update(kw)

        def ptr(x, t):
            return None if x is None else np.ascontiguousarray(x).ctypes.data_as(C.POINTER(t))
        keep = [np.ascontiguousarray(a[k]) if a[k] is not None else None
                for k in ("color", "pair_frames", "flow_ab", "flow_ba", "mask_ab", "mask_ba")]
        solver._check(fn(solver._h, C.c_int(a["num_frames"]), C.c_int(a["height"]), C.c_int(a["width"]), C.c_int(a["channels"]),
                         ptr(keep[0], C.c_float), C.c_int(a["num_pairs"]), ptr(keep[1], C.c_int32), ptr(keep[2], C.c_float),
                         ptr(keep[3], C.c_float), C.c_float(a["flow_thresh"]), C.c_float(a["color_thresh"]),
                         ptr(keep[4], C.c_uint8), ptr(keep[5], C.c_uint8), None, None, None))

    call()                                        # the unchanged arguments pass, with kept / errors / kernel_ms NULL
    assert np.array_equal(mab, run(solver, case)[0])
    for kw, msg in (({"num_frames": 0}, r"num_frames must be >= 1 \(got 0\)"),
                    ({"height": 0}, r"invalid image size: height 0, width 50"),
                    ({"width": -3}, r"invalid image size: height 31, width -3"),
                    ({"channels": 0}, r"channels must lie in \[1, 4\] \(got 0\)"),
                    ({"channels": 5}, r"channels must lie in \[1, 4\] \(got 5\)"),
                    ({"num_pairs": -1}, r"num_pairs must lie in \[0, 65535\] \(got -1\)"),
                    ({"num_pairs": 65536}, r"num_pairs must lie in \[0, 65535\] \(got 65536\)"),
                    ({"flow_thresh": -0.5}, r"flow_thresh must be finite and >= 0 \(got -0.5\)"),
                    ({"flow_thresh": float("nan")}, r"flow_thresh must be finite and >= 0 \(got nan\)"),
                    ({"color_thresh": float("inf")}, r"color_thresh must be finite and >= 0 \(got inf\)"),
                    ({"color_thresh": -1.0}, r"color_thresh must be finite and >= 0 \(got -1\)"),
                    ({"color": None}, "null color"), ({"pair_frames": None}, "null pair_frames"),
                    ({"flow_ab": None}, "null flow_ab"), ({"flow_ba": None}, "null flow_ba"),
                    ({"mask_ab": None}, "null mask_ab"), ({"mask_ba": None}, "null mask_ba"),
                    ({"pair_frames": np.array([[0, F]] + pairs[1:].tolist(), np.int32)},
                     rf"pair_frames\[0\] = \(0, {F}\) outside \[0, {F}\)"),
                    ({"pair_frames": np.array(pairs[:2].tolist() + [[-1, 2]] + pairs[3:].tolist(), np.int32)},
                     rf"pair_frames\[2\] = \(-1, 2\) outside \[0, {F}\)"),
                    ({"pair_frames": np.array([[3, 3]] + pairs[1:].tolist(), np.int32)},
                     r"pair_frames\[0\] = \(3, 3\) names one frame twice")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    before = mab.copy()
    mab[:] = 7
    call(num_pairs=0, color=None, pair_frames=None, flow_ab=None, flow_ba=None, mask_ab=None, mask_ba=None)  # returns at once
    assert (mab == 7).all()
    empty = solver.flow_consistency_masks(col, np.zeros((0, 2), np.int32), fab[:0], fba[:0])
    assert empty[0].shape == (0, H, W) and empty[2].shape == (0, 2)
    call()
    assert np.array_equal(mab, before)


def _write_dataset(base, case, directed_masks=None):
    """flow/, color_down/ (and flow_mask/ for the given directed pairs) of a case, through dataset_io.write_flow_inputs."""
    pairs = case["pairs"]
    directed = np.concatenate([pairs, pairs[:, ::-1]])
    flows = np.concatenate([case["flow_ab"], case["flow_ba"]])
    H, W = flows.shape[1:3]
    dataset_io.write_flow_inputs(base, directed, flows, np.zeros((len(directed), H, W), np.uint8), case["color"])
    for name in os.listdir(os.path.join(base, "flow_mask")):   # (write_flow_inputs writes a mask per flow: keep only the wanted)
        a, b = (int(s) for s in os.path.splitext(name)[0].split("_")[1:])
        if directed_masks is None or (a, b) not in directed_masks:
            os.remove(os.path.join(base, "flow_mask", name))
    return directed


def _png(base, a, b):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(base, "flow_mask", f"mask_{a:06d}_{b:06d}.png")))


@pytest.mark.parametrize("name", ["w50_t1_1", "w96_c1"])
def test_compute_flow_masks_on_dataset_files(solver, tmp_path, name):
    case = fc.make_case(name)
    base = str(tmp_path / "video")
    pairs = case["pairs"]
    # pair 1 already has both masks (sentinel content): it must be skipped and its files left byte-identical
    done = {tuple(pairs[1].tolist()), tuple(pairs[1][::-1].tolist())}
    _write_dataset(base, case, directed_masks=done)
    sentinel = {p: open(os.path.join(base, "flow_mask", f"mask_{p[0]:06d}_{p[1]:06d}.png"), "rb").read() for p in done}
    written = flow_masks.compute_flow_masks(base, case["flow_thresh"], case["color_thresh"], max_batch_bytes=3 * 2 * 8 * 50 * 31)
    assert written == 2 * (len(pairs) - 1)
    for p, data in sentinel.items():
        assert open(os.path.join(base, "flow_mask", f"mask_{p[0]:06d}_{p[1]:06d}.png"), "rb").read() == data
    mab, mba, kept = run(solver, case)
    for p, (a, b) in enumerate(pairs.tolist()):
        if (a, b) in done:
            continue
        got_ab, got_ba = _png(base, a, b), _png(base, b, a)
        assert got_ab.dtype == np.uint8 and got_ab.shape == mab[p].shape
        assert np.array_equal(got_ab, mab[p]) and np.array_equal(got_ba, mba[p])
        assert kept[p].tolist() == [int((got_ab > 0).sum()), int((got_ba > 0).sum())]
    assert flow_masks.compute_flow_masks(base, case["flow_thresh"], case["color_thresh"]) == 0   # nothing left to do
    # the batch size does not change a bit: one batch for everything in a fresh directory
    base2 = str(tmp_path / "video2")
    _write_dataset(base2, case, directed_masks=set())
    assert flow_masks.compute_flow_masks(base2, case["flow_thresh"], case["color_thresh"]) == 2 * len(pairs)
    for p, (a, b) in enumerate(pairs.tolist()):
        assert np.array_equal(_png(base2, a, b), mab[p]) and np.array_equal(_png(base2, b, a), mba[p])


def test_compute_flow_masks_names_the_missing_or_mismatched_file(tmp_path):
    case = fc.make_case("w50_t1_1")
    base = str(tmp_path / "video")
    _write_dataset(base, case, directed_masks=set())
    a, b = case["pairs"][2].tolist()
    reverse = os.path.join(base, "flow", f"flow_{b:06d}_{a:06d}.raw")
    keep = open(reverse, "rb").read()
    os.remove(reverse)
    with pytest.raises(FileNotFoundError, match=f"flow_{b:06d}_{a:06d}.raw"):
        flow_masks.compute_flow_masks(base)
    assert os.listdir(os.path.join(base, "flow_mask")) == []      # every input is checked before any work
    dataset_io.write_raw_image(reverse, np.zeros((20, 50, 2), np.float32))      # another size
    with pytest.raises(ValueError, match=f"flow_{b:06d}_{a:06d}.raw"):
        flow_masks.compute_flow_masks(base)
    open(reverse, "wb").write(keep)
    colour = os.path.join(base, "color_down", f"frame_{a:06d}.raw")
    os.remove(colour)
    with pytest.raises(FileNotFoundError, match=f"frame_{a:06d}.raw"):
        flow_masks.compute_flow_masks(base)


def test_pair_stats_and_the_drop_in_collection(solver, tmp_path):
    """compute_flow_pair_stats after compute_flow_masks (counts from `kept`), again in a directory whose masks are only on disk
    (counts from the PNGs), and lib_python's FlowConstraintsCollection on a dataset whose flow_mask/ and flow_list.json were both
    made by this module."""
    F, W, H = 6, 96, 56
    case = fc.make_case("w96_t1_1")
    video = synth.make_video(F, W, H, seed=3)
    base = dataset_io.write_dataset(str(tmp_path / "video"), video)
    os.remove(os.path.join(base, "flow_list.json"))
    os.remove(os.path.join(base, "flow_constraints.dat"))
    _write_dataset(base, case, directed_masks=set())
    assert flow_masks.compute_flow_masks(base) == 2 * len(case["pairs"])
    frame_pairs = [tuple(p) for p in np.asarray(video.pairs).tolist()]       # directed: every pair and its reverse
    path = flow_masks.compute_flow_pair_stats(base, frame_pairs)
    assert path == os.path.join(base, "flow_list.json")
    rows = json.load(open(path))
    mab, mba, kept = run(solver, case)
    expect, seen = [["frame0", "frame1", "mask_ratio"]], set()
    index = {tuple(p): i for i, p in enumerate(case["pairs"].tolist())}
    for a, b in frame_pairs:
        if (a, b) in seen:
            continue
        seen.update(((a, b), (b, a)))
        i = index[(min(a, b), max(a, b))]
        r = min(int(kept[i, 0]) / (H * W), int(kept[i, 1]) / (H * W))
        expect += [[a, b, r], [b, a, r]]
    assert rows == expect and len(rows) == 1 + 2 * len(case["pairs"])
    assert all(0.0 < r[2] < 1.0 for r in rows[1:])          # (long baselines keep few pixels, no pair keeps all or none)
    before = open(path, "rb").read()
    assert flow_masks.compute_flow_pair_stats(base, frame_pairs[:1]) == path and open(path, "rb").read() == before
    # counts from the PNGs: the same masks copied to a directory this process never computed
    other = str(tmp_path / "copy")
    os.makedirs(os.path.join(other, "flow_mask"))
    for name in os.listdir(os.path.join(base, "flow_mask")):
        open(os.path.join(other, "flow_mask", name), "wb").write(open(os.path.join(base, "flow_mask", name), "rb").read())
    assert json.load(open(flow_masks.compute_flow_pair_stats(other, frame_pairs))) == expect
    # the drop-in module starts from these files ("Flow list file does not exist" without flow_list.json)
    d = os.path.dirname(_b.build_lib_python())
    if d not in sys.path:
        sys.path.insert(0, d)
    lib = importlib.import_module("lib_python")
    dv = lib.DepthVideo()
    lib.DepthVideoImporter.importVideo(dv, base, True)
    fcp = lib.FlowConstraintsParams()
    fcp.frameRange.resolve(dv.numFrames(), True)
    fcp.matchSeparation = 6
    coll = lib.FlowConstraintsCollection(dv, fcp)     # no cache: samples constraints from flow/, flow_mask/, color_down/
    assert coll.numConstraints() > 40
    assert os.path.exists(os.path.join(base, "flow_constraints.dat"))
