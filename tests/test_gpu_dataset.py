"""Fine-tuning batches from the device-resident dataset on the GPU (robust_cvd_amd/csrc/cvd_batch.h) through the
numpy mirrors of api.Solver: every tensor of every recorded batch of the reference's VideoDataset
(tests/golden/reference_py/dataset_golden.npz) bit for bit -- both shapes, both N, scalar and map scales --, the host against the
device entry point, repeatability, the per-frame tables of dataset_set_xforms against the drop-in's host paramMap and warp, the
rejections, the clamp of an out-of-range device index, and the torch surface (robust_cvd_amd.video_dataset.VideoDataset) in a child
process (tests/dataset_torch_child.py).  Nothing here reads the reference tree."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from robust_cvd_amd import api, dataset_io, synth
from robust_cvd_amd.ctypes_types import SpatialXformType, ValueXformType, XformDesc
from tests import dataset_cases as dc
from tests import dataset_reference as dr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    s = api.Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(dr.GOLDEN)


def fill_store(s, config, inp, depth_orig=False):
    """The store of a configuration from the seeded arrays (what VideoDataset reads from the files), tables through set_maps."""
    _shape, temporal, recon, _depth, _list = dc.CONFIGS[config]
    pairs = dc.pairs_of(config)
    s.dataset_create(dc.F, inp["H"], inp["W"], dc.DIRECTED, pairs, temporal, depth_orig)
    s.dataset_set_colors(0, inp["colors"][:2, ..., ::-1])            # in chunks; raw colour flipped BGR -> RGB on the host
    s.dataset_set_colors(2, inp["colors"][2:, ..., ::-1])
    flows = np.stack([inp["flows"][p] for p in dc.DIRECTED])
    masks = np.stack([inp["masks"][p] for p in dc.DIRECTED])
    s.dataset_set_flows(0, flows[:5], masks[:5])
    s.dataset_set_flows(5, flows[5:], masks[5:])
    ext, intr, scales, warp = dr.pose_tables(config, inp)
    s.dataset_set_cameras(ext, intr)
    if recon != "colmap":
        s.dataset_set_maps(scales, warp)
    if depth_orig:
        with np.errstate(divide="ignore"):
            s.dataset_set_depth_orig(0, (1.0 / inp["disparity"]).astype(np.float32))
    return pairs


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for name, a in want.items():
        assert got[name].dtype == a.dtype and got[name].shape == a.shape, (what, name, got[name].shape, a.shape)
        assert got[name].tobytes() == a.tobytes(), (what, name)


@pytest.mark.parametrize("config", list(dc.CONFIGS))
def test_batches_equal_the_reference(solver, golden, config):
    inp = dc.make_inputs(config)
    pairs = fill_store(solver, config, inp)
    for idx in dc.batches_of(config):
        key = dc.batch_key(config, [pairs[i] for i in idx])
        want = {k[len(key) + 1:]: golden[k] for k in golden.files if k.startswith(key + "/")}
        assert want, key
        host = solver.dataset_batch(idx, nested=False)
        assert_same(host, want, key)
        assert_same(solver.dataset_batch(idx, nested=False, device_entry=True), host, key + " device entry")
        assert_same(solver.dataset_batch(idx, nested=False), host, key + " repeated")
    assert solver.dataset_bad_indices() == 0
    images, meta = solver.dataset_batch([0])
    assert images.shape[1] == (6 if dc.CONFIGS[config][1] else 2) and set(meta) >= {"extrinsics", "intrinsics", "geometry_consistency"}
    assert ("temporal_smoothness" in meta) == dc.CONFIGS[config][1] and ("warp" in meta) == (dc.CONFIGS[config][2] != "colmap")


def test_depth_orig_and_timing(solver):
    config = "grid_vec"
    inp = dc.make_inputs(config)
    pairs = fill_store(solver, config, inp, depth_orig=True)
    flat, ms = solver.dataset_batch([4, 1, 5], nested=False, timing=True)
    want = [pairs[i] for i in (4, 1, 5)]
    assert np.array_equal(flat["depth_orig"], dr.depth_orig(inp, want)) and flat["depth_orig"].dtype == np.float32
    assert_same({k: v for k, v in flat.items() if k != "depth_orig"}, dr.batch(config, inp, want), "with depth_orig")
    assert 0.0 < ms < 50.0, ms


def test_more_than_one_workgroup_per_plane(solver):
    """40 x 52 = 2080 pixels: three workgroups of 256 lanes x 4 pixels per plane on the 16-byte path (the last one partly idle),
    nine on the element-wise path at 41 x 51; copies of seeded planes, compared with numpy's transposes."""
    rng = np.random.default_rng(7)
    for H, W in ((40, 52), (41, 51)):
        F, pairs = 3, [(0, 1), (1, 0), (1, 2), (2, 1)]
        solver.dataset_create(F, H, W, pairs, [[0, 1], [1, 2]], True)
        color = rng.random((F, H, W, 3), np.float32)
        flow = rng.standard_normal((4, H, W, 2)).astype(np.float32)
        mask = rng.choice(np.array([0, 3], np.uint8), (4, H, W))
        scales = rng.random((F, H, W), np.float32)
        warp = rng.random((F, 2, H, W), np.float32)
        solver.dataset_set_colors(0, color)
        solver.dataset_set_flows(0, flow, mask)
        solver.dataset_set_maps(scales, warp)
        flat = solver.dataset_batch([1, 0], nested=False)
        assert flat["gc_indices"].tolist() == [[1, 2], [0, 1]] and flat["ts_indices"].tolist() == [[0, 2, 1, 2], [0, 1, 0, 2]]
        assert flat["ts_valid"].reshape(2, 2).tolist() == [[1, 0], [0, 1]]
        chw = lambda a: np.transpose(a, (2, 0, 1))
        assert np.array_equal(flat["images"][0], np.stack([chw(color[1]), chw(color[2]), chw(color[0]), chw(color[2]),
                                                             np.zeros((3, H, W), np.float32), np.zeros((3, H, W), np.float32)]))
        assert np.array_equal(flat["gc_flows0"][0], chw(flow[2])) and np.array_equal(flat["gc_flows1"][1], chw(flow[1]))
        assert np.array_equal(flat["gc_masks1"][0, 0], (mask[3] > 0).astype(np.float32))
        assert np.array_equal(flat["ts_flows0"][0], chw(flow[1])) and np.array_equal(flat["ts_flows1"][0], chw(flow[2]))
        assert np.array_equal(flat["ts_flows2"][0], np.ones((2, H, W), np.float32)) and np.array_equal(flat["ts_masks3"][0], np.ones((1, H, W), np.float32))
        assert np.array_equal(flat["ts_masks2"][1, 0], (mask[1] > 0).astype(np.float32))
        assert np.array_equal(flat["scales"][0], scales[[1, 2, 0, 2, 1, 2]]) and np.array_equal(flat["warp"][1], warp[[0, 1, 0, 1, 0, 2]])


# ---- the per-frame tables of dataset_set_xforms against the drop-in's host paramMap and warp ----------------------------------

XF, XW, XH = 3, 22, 13     # 286 pixels: two workgroups of the table kernels, an odd raster


@pytest.fixture(scope="module")
def lib():
    from robust_cvd_amd import build as _b
    d = os.path.dirname(_b.build_lib_python())
    if d not in sys.path:
        sys.path.insert(0, d)
    return importlib.import_module("lib_python")


def drop_in_maps(lib, tmp_path, depth, spatial):
    """(depth params [F, nD], spatial params [F, nS], paramMap [F, H, W] f64 or None, warp [F, H, W, 2] f32) of a lib_python
    DepthVideo whose transforms carry seeded parameters: the host functions the reference's update_poses calls per frame."""
    v = synth.make_video(XF, XW, XH, seed=11, max_pairs=2)
    base = dataset_io.write_dataset(str(tmp_path / "v"), v)
    dv = lib.DepthVideo()
    lib.DepthVideoImporter.importVideo(dv, base, True)
    dv.createDepthStream("depth_midas2", "depth_midas2", [XW, XH])
    ds = dv.depthStream(0)
    d = lib.XformDescriptor()
    d.depthType = getattr(lib.DepthXformType, depth[0])
    d.valueXform = lib.ValueXformType.Scale
    if depth[0] == "Grid":
        d.gridSize = [depth[1], depth[2], 1]
        d.cubicInterpolation = depth[3]
    ds.resetDepthXforms(d)
    sd = lib.XformDescriptor()
    sd.reset(lib.XformType.Spatial)
    sd.spatialType = getattr(lib.SpatialXformType, spatial[0])
    if len(spatial) > 1:
        sd.gridSize = [spatial[1], spatial[2], 0]
    ds.resetSpatialXforms(sd)
    rng = np.random.default_rng(13)
    dp, sp, pmap, warp = [], [], [], []
    for f in range(XF):
        fr = ds.frame(f)
        n = fr.depthXform().numParams()
        if n:
            fr.depthXform().setParams((0.5 + rng.random(n)).tolist())
        m = fr.spatialXform().numParams()
        if m:
            fr.spatialXform().setParams((0.05 * rng.standard_normal(m)).tolist())
        dp.append(np.asarray(fr.depthXform().params(), np.float64))
        sp.append(np.asarray(fr.spatialXform().params(), np.float64))
        if depth[0] == "Grid":
            pmap.append(np.asarray(fr.depthXform().paramMap(fr)))
        warp.append(np.asarray(fr.spatialXform().warp(XH, XW), np.float32))
    return np.stack(dp), np.stack(sp), np.stack(pmap) if pmap else None, np.stack(warp)


def xform_store(solver):
    solver.dataset_create(XF, XH, XW, [(0, 1), (1, 0), (1, 2), (2, 1)], [[0, 1], [1, 2]], True)


@pytest.mark.parametrize("depth,spatial,ddesc,sdesc", [
    (("Grid", 5, 4, False), ("BilinearGrid", 4, 3), XformDesc.grid_depth(5, 4), XformDesc.spatial(SpatialXformType.BilinearGrid, 4, 3)),
    (("Grid", 5, 4, True), ("BicubicGrid", 4, 3), XformDesc.grid_depth(5, 4, cubic=True),
     XformDesc.spatial(SpatialXformType.BicubicGrid, 4, 3)),
    (("Grid", 3, 2, False), ("CornersBilinear",), XformDesc.grid_depth(3, 2), XformDesc.spatial(SpatialXformType.CornersBilinear)),
    (("Grid", 2, 2, False), ("VerticalLinear",), XformDesc.grid_depth(2, 2), XformDesc.spatial(SpatialXformType.VerticalLinear)),
], ids=["linear-bilinear", "cubic-bicubic", "linear-corners", "linear-vertical"])
def test_set_xforms_against_the_drop_in_host_maps(solver, lib, tmp_path, depth, spatial, ddesc, sdesc):
    dp, sp, pmap, warp = drop_in_maps(lib, tmp_path, depth, spatial)
    xform_store(solver)
    solver.dataset_set_xforms(ddesc, dp, sdesc, sp)
    flat = solver.dataset_batch([0, 1], nested=False)
    frames = [[0, 1, 0, 1, 0, 2], [1, 2, 0, 2, 1, 2]]
    assert flat["scales"].shape == (2, 6, XH, XW) and flat["warp"].shape == (2, 6, 2, XH, XW)
    for b in range(2):
        # f32 storage of identical f64 sums: the bars of tests/test_gpu_dense_maps.py
        np.testing.assert_allclose(flat["scales"][b], pmap.astype(np.float32)[frames[b]], rtol=2e-7, atol=0)
        np.testing.assert_allclose(flat["warp"][b], np.transpose(warp, (0, 3, 1, 2))[frames[b]], rtol=2e-7, atol=1e-12)
    assert np.abs(warp).max() > 1e-3 and np.ptp(pmap) > 0.1


def test_set_xforms_identity_and_global_scalars(solver, lib, tmp_path):
    xform_store(solver)
    solver.dataset_set_xforms(XformDesc.identity_depth(), None, XformDesc.spatial(), None)
    flat = solver.dataset_batch([1], nested=False)
    assert flat["scales"].shape == (1, 6, 1, 1) and np.array_equal(flat["scales"].ravel(), np.ones(6, np.float32))
    assert not flat["warp"].any()
    theta = np.array([[1.25], [0.1], [3.000000001]])
    solver.dataset_set_xforms(XformDesc.global_depth(), theta, XformDesc.spatial(), None)
    flat = solver.dataset_batch([1], nested=False)
    assert np.array_equal(flat["scales"].ravel(), theta.astype(np.float32).ravel()[[1, 2, 0, 2, 1, 2]])
    # the drop-in's Global transform hands update_poses the same scalar
    dp, _sp, _pmap, warp = drop_in_maps(lib, tmp_path, ("Global",), ("Identity",))
    solver.dataset_set_xforms(XformDesc.global_depth(), dp, XformDesc.spatial(), None)
    assert np.array_equal(solver.dataset_batch([0], nested=False)["scales"].ravel(), dp.astype(np.float32).ravel()[[0, 1, 0, 1, 0, 2]])
    assert not warp.any()


# ---- rejections, each with its message and before any device work ------------------------------------------------------------

def test_create_rejections(solver):
    solver.dataset_clear()
    good = dict(num_frames=3, height=4, width=4, pair_frames=[(0, 1), (1, 0), (1, 2), (2, 1)], samples=[[0, 1]], temporal=False)

    def create(**kw):
        solver.dataset_create(**{**good, **kw})
    for kw, msg in (
            (dict(pair_frames=[(0, 1), (1, 3)], samples=[]), r"frame 3 of pair 1 is out of range \[0, 3\)"),
            (dict(pair_frames=[(0, 1), (-1, 0)], samples=[]), "frame -1 of pair 1 is out of range"),
            (dict(pair_frames=[(0, 1), (1, 0), (0, 1)]), r"directed pair \(0, 1\) is listed twice"),
            (dict(pair_frames=[(0, 1), (1, 2), (2, 1)]), r"sample 0 \(0, 1\): direction \(1, 0\) is not in the pair list"),
            (dict(samples=[[0, 2]]), r"sample 0 \(0, 2\): direction \(0, 2\) is not in the pair list"),
            (dict(samples=[[0, 5]]), "frame 5 of sample 0 is out of range"),
            (dict(pair_frames=[(1, 2), (2, 1)], samples=[[1, 2]], temporal=True),
             r"temporal sample 0: neighbour flow \(1, 0\) of interior frame 1 is not in the pair list"),
            (dict(pair_frames=[(0, 1), (1, 0)], temporal=True), r"temporal sample 0: neighbour flow \(1, 2\) of interior frame 1"),
            (dict(height=0), "invalid shape"),
            (dict(neighbor_rule_frames=4), "neighbor_rule_frames 4 exceeds"),
    ):
        with pytest.raises(RuntimeError, match=msg):
            create(**kw)
        with pytest.raises(RuntimeError, match="no store"):      # nothing was created
            solver.dataset_batch([0])
    # a stale struct_size
    for stale in (C.sizeof(api.DatasetDesc), (C.sizeof(api.DatasetDesc) - 4) | (api.ABI_REVISION << 32),
                  C.sizeof(api.DatasetDesc) | ((api.ABI_REVISION - 1) << 32)):
        d = api.dataset_desc(3, 4, 4, 4, 1, False)
        d.struct_size = stale
        with pytest.raises(RuntimeError, match="struct_size"):
            create(desc=d)
    with pytest.raises(RuntimeError, match="no store"):
        solver.dataset_set_colors(0, np.zeros((1, 1, 1, 3), np.float32))
    with pytest.raises(RuntimeError, match="no store"):
        solver.dataset_bad_indices()


def test_batch_and_upload_rejections(solver):
    fill_store(solver, "grid_vec", dc.make_inputs("grid_vec"))
    S = len(dc.pairs_of("grid_vec"))
    before = solver.dataset_batch([0], nested=False)
    for bad in ([S], [0, -1], [2 ** 40]):
        with pytest.raises(RuntimeError, match=r"indices\[\d\] = -?\d+ is outside the store's 6 samples"):
            solver.dataset_batch(bad)
    with pytest.raises(RuntimeError, match="batch size must be >= 1"):
        solver.dataset_batch([])
    lib = api.load_library()
    idx = np.zeros(1, np.int64)
    ip = idx.ctypes.data_as(C.POINTER(C.c_int64))
    err = lambda: lib.cvd_last_error(solver._h).decode()
    shapes = api.dataset_batch_shapes(1, 6, 4, 8, 2, True)
    arrays = {k: np.zeros(shape, dtype) for k, (shape, dtype) in shapes.items()}
    for missing in ("images", "gc_flows1", "ts_masks3", "ts_valid", "intrinsics"):
        out = api.dataset_batch_out({k: a.ctypes.data for k, a in arrays.items() if k != missing})
        assert solver._fn("dataset_batch")(solver._h, C.c_int32(1), ip, C.byref(out), None) != 0
        assert f"null output {missing[:-1] + '[' + missing[-1] + ']' if missing[-1].isdigit() else missing}" in err(), err()
        assert solver._fn("dataset_batch_device")(solver._h, C.c_int32(1), ip, C.byref(out), None) != 0 and "null output" in err()
    out = api.dataset_batch_out({k: a.ctypes.data for k, a in arrays.items()})
    assert solver._fn("dataset_batch")(solver._h, C.c_int32(1), None, C.byref(out), None) != 0 and "null indices" in err()
    assert solver._fn("dataset_batch")(solver._h, C.c_int32(1), ip, None, None) != 0 and "null out" in err()
    out.struct_size -= 8
    assert solver._fn("dataset_batch")(solver._h, C.c_int32(1), ip, C.byref(out), None) != 0 and "struct_size" in err()
    out = api.dataset_batch_out({**{k: a.ctypes.data for k, a in arrays.items()}, "depth_orig": arrays["images"].ctypes.data})
    assert solver._fn("dataset_batch")(solver._h, C.c_int32(1), ip, C.byref(out), None) != 0 and "created without it" in err()
    assert not any(a.any() for a in arrays.values())
    with pytest.raises(RuntimeError, match=r"frames \[4, 4 \+ 2\) leave the store's 5"):
        solver.dataset_set_colors(4, np.zeros((2, 4, 8, 3), np.float32))
    with pytest.raises(RuntimeError, match=r"pairs \[14, 14 \+ 1\) leave the store's 14"):
        solver.dataset_set_flows(14, np.zeros((1, 4, 8, 2), np.float32), np.zeros((1, 4, 8), np.uint8))
    with pytest.raises(RuntimeError, match="created without depth_orig"):
        solver.dataset_set_depth_orig(0, np.zeros((1, 4, 8), np.float32))
    assert_same(solver.dataset_batch([0], nested=False), before, "after the rejections")


def test_xform_rejections(solver):
    """What the reference's update_poses refuses (loaders/video_dataset.py:195-217), and the depth-wise grid."""
    fill_store(solver, "grid_vec", dc.make_inputs("grid_vec"))
    before = solver.dataset_batch([3], nested=False)
    sp = XformDesc.spatial()
    theta = np.ones((dc.F, 8))
    for dd, sd, msg in (
            (XformDesc.global_depth(ValueXformType.ScaleShift), sp, "We only support scale-based transforms at the moment."),
            (XformDesc.grid_depth(2, 2, ValueXformType.ScaleShift), sp, "We only support scale-based transforms"),
            (XformDesc(type=0, depth_type=0, value_xform=1), sp, "Unsupported depth transform type '0'"),
            (XformDesc(type=0, depth_type=7, value_xform=1), sp, "Unsupported depth transform type '7'"),
            (XformDesc.global_depth(), XformDesc.spatial(SpatialXformType.NONE), "Unsupported spatial transform type '0'"),
            (XformDesc.global_depth(), XformDesc(type=1, spatial_type=9), "Unsupported spatial transform type '9'"),
            (XformDesc.grid_depth(2, 2, depth=2, dmin=0.5, dmax=2.0), sp, "depth-wise grid"),
            (XformDesc.grid_depth(1, 2), sp, "at least two rows and columns"),
    ):
        with pytest.raises(RuntimeError, match=msg):
            solver.dataset_set_xforms(dd, theta, sd, None)
    with pytest.raises(RuntimeError, match="null parameters"):
        solver.dataset_set_xforms(XformDesc.global_depth(), None, sp, None)
    assert_same(solver.dataset_batch([3], nested=False), before, "after the rejections")    # the tables stay


def test_device_entry_clamps_and_counts_an_out_of_range_index(solver):
    config = "grid_odd"
    inp = dc.make_inputs(config)
    pairs = fill_store(solver, config, inp)
    S = len(pairs)
    assert solver.dataset_bad_indices() == 0
    got = solver.dataset_batch([1, S + 3, 2], nested=False, device_entry=True)
    assert_same(got, dr.batch(config, inp, [pairs[1], pairs[S - 1], pairs[2]]), "clamped")
    assert solver.dataset_bad_indices() == 1
    got = solver.dataset_batch([-5, 0], nested=False, device_entry=True)
    assert_same(got, dr.batch(config, inp, [pairs[0], pairs[0]]), "clamped from below")
    assert solver.dataset_bad_indices() == 2
    solver.dataset_batch([0, 1], device_entry=True)
    assert solver.dataset_bad_indices() == 2


def test_store_is_replaced_and_cleared(solver):
    inp = dc.make_inputs("grid_vec")
    fill_store(solver, "grid_vec", inp)
    a = solver.dataset_batch([0, 5], nested=False)
    inp2 = dc.make_inputs("colmap_odd")
    pairs = fill_store(solver, "colmap_odd", inp2)                 # another shape, N = 2, no tables
    b = solver.dataset_batch([5, 0], nested=False)
    assert_same(b, dr.batch("colmap_odd", inp2, [pairs[5], pairs[0]]), "second store")
    assert "ts_indices" not in b and "scales" not in b and b["images"].shape == (2, 2, 3, 5, 6)
    fill_store(solver, "grid_vec", inp)
    assert_same(solver.dataset_batch([0, 5], nested=False), a, "first store again")
    solver.dataset_clear()
    with pytest.raises(RuntimeError, match="no store"):
        solver.dataset_batch([0])
    solver.dataset_clear()                                          # (clearing nothing is fine)
    other = api.Solver(0)                                           # cvd_destroy frees a live store
    fill_store(other, "grid_odd", dc.make_inputs("grid_odd"))
    other.close()


def test_torch_surface():
    """robust_cvd_amd.video_dataset.VideoDataset on GPU tensors, in a fresh process: torch has to be imported before libcvd_hip.so
    is loaded (the process then holds one HIP runtime, torch's).  The checks are tests/dataset_torch_child.py's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.dataset_torch_child"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch dataset ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
