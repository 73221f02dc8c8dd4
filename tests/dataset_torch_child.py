"""Child process of tests/test_gpu_dataset.py::test_torch_surface (python -m tests.dataset_torch_child): torch is imported first,
then the library.  robust_cvd_amd.video_dataset.VideoDataset on the dataset directories of tests/dataset_cases.py (regenerated from
the seed): batches against the reference's recorded run, the loader's epochs, depth_orig, update_poses on the device against its
host path on a lib_python DepthVideo, one launch and no host wait per batch, a batch through JointLoss, and the error cases."""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

from robust_cvd_amd import api, dataset_io, synth
from robust_cvd_amd import torch_common as tc
from robust_cvd_amd.joint_loss import JointLoss
from robust_cvd_amd.video_dataset import VideoDataset
from tests import dataset_cases as dc
from tests import dataset_reference as dr
from tests import spatial_cases as sc

DEV = torch.device("cuda", 0)


def flat_of(images, meta):
    out = {"images": images, "extrinsics": meta["extrinsics"], "intrinsics": meta["intrinsics"],
           "gc_indices": meta["geometry_consistency"]["indices"]}
    for d in range(2):
        out[f"gc_flows{d}"], out[f"gc_masks{d}"] = meta["geometry_consistency"]["flows"][d], meta["geometry_consistency"]["masks"][d]
    if "temporal_smoothness" in meta:
        ts = meta["temporal_smoothness"]
        out["ts_indices"], out["ts_valid"] = ts["indices"], ts["valid"]
        for d in range(4):
            out[f"ts_flows{d}"], out[f"ts_masks{d}"] = ts["flows"][d], ts["masks"][d]
    for k in ("scales", "warp", "depth_orig"):
        if k in meta:
            out[k] = meta[k]
    for k, t in out.items():
        assert t.device == DEV and t.is_contiguous(), k
    return {k: t.cpu().numpy() for k, t in out.items()}


def same(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k, a in want.items():
        assert got[k].dtype == a.dtype and got[k].shape == a.shape and got[k].tobytes() == a.tobytes(), (what, k)


def make(config, tmp, initial_depth=False):
    inp = dc.make_inputs(config)
    path, meta, depth_dir = dc.write_dataset(config, os.path.join(tmp, config), inp, initial_depth)
    _shape, temporal, recon, _depth, _list = dc.CONFIGS[config]
    ds = VideoDataset(path, dc.FRAMES, dc.MIN_MASK_RATIO, temporal, meta, recon, device=DEV, initial_depth_dir=depth_dir)
    if recon != "colmap":
        ds.update_poses(dc.Replay(config, inp), host_maps=True)      # (the replay's maps are seeded arrays: the host path)
    return ds, inp


def check_fixture(tmp, golden):
    for config in dc.CONFIGS:
        ds, _inp = make(config, tmp)
        pairs = dc.pairs_of(config)
        assert ds.flow_indices == pairs and len(ds) == len(pairs)
        for idx in dc.batches_of(config):
            key = dc.batch_key(config, [pairs[i] for i in idx])
            want = {k[len(key) + 1:]: golden[k] for k in golden.files if k.startswith(key + "/")}
            same(flat_of(*ds.batch(idx)), want, key)
            same(flat_of(*ds.batch(torch.tensor(idx))), want, key + " (CPU tensor)")
            same(flat_of(*ds.batch(torch.tensor(idx, device=DEV, dtype=torch.int32))), want, key + " (device tensor)")
        # one sample: the reference's per-sample shapes
        images, meta = ds[1]
        key = dc.batch_key(config, [pairs[1]])
        one = {k: v[0] for k, v in dr.batch(config, dc.make_inputs(config), [pairs[1]]).items()}
        same(flat_of(images, meta), one, key + " __getitem__")
    assert tc.solver(DEV).dataset_bad_indices() == 0


def check_loader_and_depth_orig(tmp):
    config = "nolist_vec"                                   # seven samples
    ds, inp = make(config, tmp, initial_depth=True)
    pairs = dc.pairs_of(config)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    orders = []
    for _epoch in range(2):
        seen = []
        sizes = []
        for images, meta in ds.loader(3, shuffle=True, generator=gen):
            idx = meta["geometry_consistency"]["indices"].cpu().tolist()
            sizes.append(len(idx))
            seen += idx
            want = dr.batch(config, inp, idx)
            want["depth_orig"] = dr.depth_orig(inp, idx)
            same(flat_of(images, meta), want, f"loader {idx}")
        assert sizes == [3, 3, 1] and sorted(seen) == pairs, (sizes, seen)        # every sample once, a short last batch
        orders.append(seen)
    assert orders[0] != pairs or orders[1] != pairs                               # shuffled
    assert [m["geometry_consistency"]["indices"].shape[0] for _i, m in ds.loader(3, drop_last=True)] == [3, 3]
    assert torch.cat([m["geometry_consistency"]["indices"] for _i, m in ds.loader(4)]).cpu().tolist() == pairs
    gen.manual_seed(5)
    again = [m["geometry_consistency"]["indices"].cpu().tolist() for _i, m in ds.loader(3, shuffle=True, generator=gen)]
    assert sum(again, []) == orders[0]                                            # the seed decides the order


class CallCounter:
    def __init__(self, solver):
        self.names, self.fn = [], solver._fn
        solver._fn = self

    def __call__(self, name, *args, **kw):
        self.names.append(name)
        return self.fn(name, *args, **kw)


def check_one_enqueued_call_per_batch(tmp):
    ds, _inp = make("grid_vec", tmp)
    solver = tc.solver(DEV)
    idx = torch.tensor([0, 3, 5], device=DEV)
    ds.batch(idx)
    torch.cuda.synchronize()
    counter = CallCounter(solver)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        images, meta = ds.batch(idx)            # on torch's current stream
    solver._fn = counter.fn
    assert counter.names == ["dataset_batch_device"], counter.names
    side.synchronize()
    assert torch.equal(meta["geometry_consistency"]["indices"].cpu(), torch.tensor(dc.pairs_of("grid_vec"))[[0, 3, 5]])


def lib_python():
    from robust_cvd_amd import build as _b
    d = os.path.dirname(_b.build_lib_python())
    if d not in sys.path:
        sys.path.insert(0, d)
    return importlib.import_module("lib_python")


def check_update_poses_on_a_depth_video(tmp):
    """update_poses on the drop-in's DepthVideo: the tables filled on the device equal the reference's per-frame host path (f32
    storage of identical f64 sums: rtol 2e-7, the bar of tests/test_gpu_dense_maps.py), the cameras bit for bit."""
    lib = lib_python()
    config = "grid_vec"
    inp = dc.make_inputs(config)
    H, W = inp["H"], inp["W"]
    path, _meta, _ = dc.write_dataset(config, os.path.join(tmp, "dv_data"), inp)
    v = synth.make_video(dc.F, W, H, seed=3, max_pairs=2)
    base = dataset_io.write_dataset(os.path.join(tmp, "dv"), v)
    dv = lib.DepthVideo()
    lib.DepthVideoImporter.importVideo(dv, base, True)
    dv.createDepthStream("depth_midas2", "depth_midas2", [W, H])
    stream = dv.depthStream(0)
    d = lib.XformDescriptor()
    d.depthType, d.valueXform, d.gridSize, d.cubicInterpolation = lib.DepthXformType.Grid, lib.ValueXformType.Scale, [4, 3, 1], True
    stream.resetDepthXforms(d)
    sd = lib.XformDescriptor()
    sd.reset(lib.XformType.Spatial)
    sd.spatialType, sd.gridSize = lib.SpatialXformType.BicubicGrid, [4, 3, 0]
    stream.resetSpatialXforms(sd)
    rng = np.random.default_rng(17)
    for f in range(dc.F):
        fr = stream.frame(f)
        fr.depthXform().setParams((0.5 + rng.random(fr.depthXform().numParams())).tolist())
        fr.spatialXform().setParams((0.05 * rng.standard_normal(fr.spatialXform().numParams())).tolist())
        fr.extrinsics.position = rng.standard_normal(3).astype(np.float32).tolist()
    ds = VideoDataset(path, dc.FRAMES, dc.MIN_MASK_RATIO, True, None, "i3d", device=DEV)
    idx = list(range(len(ds)))
    ds.update_poses(dv, host_maps=True)
    host = flat_of(*ds.batch(idx))
    ds.update_poses(dv)
    dev = flat_of(*ds.batch(idx))
    assert np.ptp(host["scales"]) > 0.1 and np.abs(host["warp"]).max() > 1e-3
    np.testing.assert_allclose(dev["scales"], host["scales"], rtol=2e-7, atol=0)
    np.testing.assert_allclose(dev["warp"], host["warp"], rtol=2e-7, atol=1e-12)
    for k in host:
        if k not in ("scales", "warp"):
            assert dev[k].tobytes() == host[k].tobytes(), k
    # the cameras are the getters' values, as the reference stacks them
    a, b = dc.pairs_of(config)[2]
    fr = stream.frame(a)
    assert host["extrinsics"][2, 0, :, 3].tolist() == np.asarray(fr.extrinsics.position, np.float32).tolist()
    assert host["extrinsics"][2, 0, :, 0].tolist() == np.asarray(fr.extrinsics.right(), np.float32).tolist()
    assert host["intrinsics"][2, 0, 2:].tolist() == [W / 2.0, H / 2.0]


def check_joint_loss(tmp):
    """A batch (N = 6, every term on) through this package's JointLoss and back: it runs and is finite."""
    config = "grid_vec"
    inp = dc.make_inputs(config)
    # cameras that look down -z from nearly one place, so that every reprojection is well defined
    for k, axis in (("right", [1, 0, 0]), ("up", [0, 1, 0]), ("backward", [0, 0, 1])):
        inp[k] = np.tile(np.array(axis, np.float32), (dc.F, 1))
    inp["position"] = inp["position"] / 256
    path, _meta, depth_dir = dc.write_dataset(config, os.path.join(tmp, config), inp, True)
    ds = VideoDataset(path, dc.FRAMES, dc.MIN_MASK_RATIO, True, None, "i3d", device=DEV, initial_depth_dir=depth_dir)
    ds.update_poses(dc.Replay(config, inp), host_maps=True)
    images, meta = ds.batch([1, 4, 0])
    B, N, _c, H, W = images.shape
    opt = types.SimpleNamespace(**dict(sc.JOINT_OPTIONS, recon="i3d", lambda_parameter=0.0))
    torch.manual_seed(3)
    depths = (1.0 + torch.rand(B, N, H, W, device=DEV)).requires_grad_(True)
    depths_orig = torch.cat([meta["depth_orig"], torch.ones(B, N - 2, H, W, device=DEV)], dim=1)
    keep = meta["warp"].clone()
    loss, batch_losses, _scene_flow = JointLoss(opt)(images, depths_orig, depths, meta)
    loss.sum().backward()
    assert torch.isfinite(loss).all() and torch.isfinite(depths.grad).all() and depths.grad.abs().sum() > 0
    assert batch_losses and all(torch.isfinite(v).all() for v in batch_losses.values())
    assert torch.equal(meta["warp"], keep)


def check_errors(tmp):
    def raises(exc, text, fn):
        try:
            fn()
        except exc as e:
            assert text in str(e), (text, str(e))
            return
        raise AssertionError(f"{exc.__name__}({text!r}) not raised")
    ds, inp = make("grid_vec", tmp)
    raises(IndexError, "index out of range", lambda: ds.batch([0, len(ds)]))
    raises(IndexError, "index out of range", lambda: ds.batch(torch.tensor([-1])))
    raises(ValueError, "empty batch", lambda: ds.batch([]))
    raises(ValueError, "no CPU path", lambda: VideoDataset("x", [0], None, False, device="cpu"))
    path = os.path.join(tmp, "grid_vec")
    fresh = VideoDataset(path, dc.FRAMES, dc.MIN_MASK_RATIO, True, None, "i3d", device=DEV)
    raises(RuntimeError, "call update_poses first", lambda: fresh.batch([0]))
    replay = dc.Replay("grid_vec", inp)
    replay.depth = "Global"
    frame = replay.frame

    def shift(i):
        f = frame(i)
        f.depthXform().desc().valueXform = dc.ValueXformType.ScaleShift
        return f
    replay.frame = shift
    raises(AssertionError, "", lambda: fresh.update_poses(replay))
    os.remove(os.path.join(path, "color_down", "frame_000004.raw"))
    raises(FileNotFoundError, "frame_000004.raw", lambda: VideoDataset(path, dc.FRAMES, dc.MIN_MASK_RATIO, True, None, "i3d", device=DEV))
    # a device index out of range is clamped and counted, never read through
    solver = tc.solver(DEV)
    ds2, inp2 = make("grid_odd", tmp)
    before = solver.dataset_bad_indices()
    got = flat_of(*ds2.batch(torch.tensor([len(ds2) + 3], device=DEV)))
    same(got, dr.batch("grid_odd", inp2, [dc.pairs_of("grid_odd")[-1]]), "clamped")
    assert solver.dataset_bad_indices() == before + 1


def main():
    golden = np.load(dr.GOLDEN)
    with tempfile.TemporaryDirectory() as tmp:
        check_fixture(os.path.join(tmp, "a"), golden)
        check_loader_and_depth_orig(os.path.join(tmp, "b"))
        check_one_enqueued_call_per_batch(os.path.join(tmp, "c"))
        check_update_poses_on_a_depth_video(os.path.join(tmp, "d"))
        check_joint_loss(os.path.join(tmp, "e"))
        check_errors(os.path.join(tmp, "f"))
    print("torch dataset ok")


if __name__ == "__main__":
    main()
