"""Drop-in for the reference's `loaders/video_dataset.py::VideoDataset`, the DataLoaders around it and `to_device`: the dataset's
colour, flow and mask images are read ONCE and kept on the GPU in their file layout, and a batch is one HIP kernel launch that
writes every tensor of it in the layout the losses read (csrc/cvd_batch.h).

    from robust_cvd_amd.video_dataset import VideoDataset
    dataset = VideoDataset(path, frames, min_mask_ratio, use_temporal_smooth_loss, meta_file, recon,
                           device="cuda", initial_depth_dir=None)   # the reference's six arguments, then two extensions
    dataset.update_poses(pose_optimizer.depth_video)                # after every pose optimisation, as in the reference
    for images, metadata in dataset.loader(batch_size, shuffle=True):    # replaces both DataLoaders and to_device
        ...

`images` (B, N, 3, H, W) and `metadata` carry the reference's nesting, key names, shapes and values: "extrinsics", "intrinsics",
"geometry_consistency" {"indices", "flows", "masks"}, "temporal_smoothness" {"indices", "flows", "masks", "valid"} with
use_temporal_smooth_loss, "scales" after update_poses, "warp" unless recon == "colmap", and "depth_orig" (B, 2, H, W) when
`initial_depth_dir` names a directory of frame_%06d.raw disparity files (what depth_fine_tuning.py's retrieve_depth_orig and its
view(-1, 2, h, w) produce).  All are tensors on `device`; a batch is enqueued on torch's current stream with no host
synchronisation.  update_poses fills the per-frame scale maps and warps on the GPU from the transforms' parameters, one launch
per table, instead of calling paramMap and warp per frame on the host.

Differences from the reference:
  * The sample order.  The reference's is the iteration order of a Python set of named tuples, an artefact of the process; here
    the one-way pairs are sorted.  (A pair still survives when either of its directions passes the score test.)
  * A missing colour, flow or mask file raises FileNotFoundError at construction, not in the middle of an epoch.
  * `loader(...)` replaces `torch.utils.data.DataLoader(dataset, ...)` and `to_device`; there are no worker processes.
  * update_poses(depth_video, host_maps=True) takes the reference's per-frame host path; a depth-wise grid (grid z > 1), whose map
    needs the source depth, always does.
  * The store belongs to the per-device handle of robust_cvd_amd.torch_common: one VideoDataset per device at a time, and calls on
    one device are ordered on one stream (or synchronised across streams), as for the loss modules.

`plan` holds everything that decides which files are read, and needs no GPU.  Import this module (torch) before anything loads
libcvd_hip.so.
"""
import json
import math
import os
from os.path import join as pjoin

import numpy as np

from . import dataset_io

CHUNK_BYTES = 64 << 20   # host staging of one upload call


def to_one_way(pairs):
    """reference utils/frame_sampling.py:140-146, as a sorted list"""
    return sorted({(min(a, b), max(a, b)) for a, b in pairs})


def plan(path, frames, min_mask_ratio, use_temporal_smooth_loss):
    """What the reference's constructor and __getitem__ decide about files (loaders/video_dataset.py:104-147, 223-245, 309-328),
    without reading an image: {"color_fmt", "flow_fmt", "mask_fmt", "pairs": sorted one-way sample pairs, "directed": the
    directed pairs whose flow and mask are read, "color_frames": sorted frames whose colour is read, "num_frames": len(frames)}.
    Raises FileNotFoundError naming the first missing flow, mask or colour file."""
    frames = list(frames)
    color_fmt = pjoin(path, "color_down", "frame_{:06d}.raw")
    if not os.path.isfile(color_fmt.format(0)):
        color_fmt = pjoin(path, "color_down", "frame_{:06d}.png")
    mask_fmt = pjoin(path, "flow_mask", "mask_{:06d}_{:06d}.png")
    flow_fmt = pjoin(path, "flow", "flow_{:06d}_{:06d}.raw")
    flow_list_fn = pjoin(path, "flow_list.json")
    if os.path.isfile(flow_list_fn):
        with open(flow_list_fn, "r") as f:
            rows = json.load(f)
        # strip the header, drop pairs with low overlap or a frame outside `frames`
        indices = [[f0, f1] for f0, f1, score in rows[1:]
                   if f0 in frames and f1 in frames and (min_mask_ratio is None or score > min_mask_ratio)]
    else:
        ext = os.path.splitext(flow_fmt)[-1]
        indices = [[int(s) for s in os.path.splitext(name)[0].split("_")[-2:]]
                   for name in sorted(os.listdir(os.path.dirname(flow_fmt))) if os.path.splitext(name)[-1] == ext]
    pairs = to_one_way(indices)
    num_frames = len(frames)
    directed, color_frames = [], set()
    for a, b in pairs:
        directed += [(a, b), (b, a)]
        color_frames |= {a, b}
        if use_temporal_smooth_loss:
            for k in (a, b):
                if 0 < k < num_frames - 1:
                    directed += [(k, k - 1), (k, k + 1)]
                    color_frames |= {k - 1, k + 1}
    directed = sorted(set(directed))
    for a, b in directed:
        for fn in (flow_fmt.format(a, b), mask_fmt.format(a, b)):
            if not os.path.isfile(fn):
                raise FileNotFoundError(fn)
    for k in sorted(color_frames):
        if not os.path.isfile(color_fmt.format(k)):
            raise FileNotFoundError(color_fmt.format(k))
    return {"color_fmt": color_fmt, "flow_fmt": flow_fmt, "mask_fmt": mask_fmt, "pairs": [list(p) for p in pairs],
            "directed": [list(p) for p in directed], "color_frames": sorted(color_frames), "num_frames": num_frames}


def load_color(path):
    """float32 [H, W, 3] in the channel order the reference's load_color returns (loaders/video_dataset.py:49-60): a raw file is
    flipped BGR -> RGB; any other file is what cv2.imread gives (BGR, not flipped) / 255.  Pillow decodes RGB where cv2 gives BGR,
    so its result is reversed once."""
    if os.path.splitext(path)[-1] == ".raw":
        im = dataset_io.read_raw_image(path)
        return np.ascontiguousarray(im[..., [2, 1, 0]] if im.ndim == 3 else im, dtype=np.float32)
    from PIL import Image
    im = np.asarray(Image.open(path))
    if im.ndim == 3:
        im = im[..., ::-1]
    return np.ascontiguousarray(im / 255, dtype=np.float32)


def load_mask(path):
    """uint8 [H, W] as stored (nonzero counts as 1)"""
    from PIL import Image
    im = np.asarray(Image.open(path))
    if im.ndim != 2:
        raise ValueError(f"receive image of shape {im.shape} whose #channels != 1")
    return np.ascontiguousarray(im, dtype=np.uint8)


def load_flow(path):
    fl = dataset_io.read_raw_image(path)
    if fl.ndim != 3 or fl.shape[2] != 2:
        raise ValueError(f"receive image of shape {fl.shape} whose #channels != 2")
    return fl


def cameras_of(depth_video, frames):
    """(extrinsics [N, 3, 4], intrinsics [N, 4]) float32 exactly as the reference's update_poses forms them
    (loaders/video_dataset.py:159-189): the getters' floats into float32 rows, the focal lengths in Python floats."""
    N = depth_video.numFrames()
    ds = depth_video.depthStream(depth_video.numDepthStreams() - 1)
    ext = np.zeros((N, 3, 4), np.float32)
    intr = np.zeros((N, 4), np.float32)
    for i in frames:
        f = ds.frame(i)
        ext[i, :, 0] = f.extrinsics.right()
        ext[i, :, 1] = f.extrinsics.up()
        ext[i, :, 2] = f.extrinsics.backward()
        ext[i, :, 3] = f.extrinsics.position
        W = ds.width() / 2.0
        H = ds.height() / 2.0
        intr[i, 0] = W / math.tan(f.intrinsics.hFov / 2.0)
        intr[i, 1] = H / math.tan(f.intrinsics.vFov / 2.0)
        intr[i, 2] = W
        intr[i, 3] = H
    return ext, intr


_VALID_SPATIAL = ("Identity", "VerticalLinear", "CornersBilinear", "BilinearGrid", "BicubicGrid")


def _xform_desc(desc):
    """The ctypes descriptor of a lib_python.XformDescriptor (its enums convert with int())."""
    from .ctypes_types import XformDesc
    d = XformDesc(type=int(desc.type), depth_type=int(getattr(desc, "depthType", 0)), spatial_type=int(getattr(desc, "spatialType", 0)),
                  value_xform=int(getattr(desc, "valueXform", 0)), cubic_interpolation=int(bool(getattr(desc, "cubicInterpolation", False))))
    grid = list(getattr(desc, "gridSize", (0, 0, 0)))
    for k in range(3):
        d.grid_size[k] = int(grid[k])
    mm = list(getattr(desc, "depthMinMax", (0.0, 0.0)))
    d.depth_min_max[0], d.depth_min_max[1] = float(mm[0]), float(mm[1])
    return d


class VideoDataset:
    def __init__(self, path, frames, min_mask_ratio, use_temporal_smooth_loss, meta_file=None, recon=None, device="cuda",
                 initial_depth_dir=None):
        import torch
        from . import torch_common as tc
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("VideoDataset keeps its data on a GPU: there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.recon = recon
        self.use_temporal_smooth_loss = bool(use_temporal_smooth_loss)
        self.frames = list(frames)
        self.num_frames = len(self.frames)
        p = plan(path, self.frames, min_mask_ratio, self.use_temporal_smooth_loss)
        self.color_fmt, self.flow_fmt, self.mask_fmt = p["color_fmt"], p["flow_fmt"], p["mask_fmt"]
        self.flow_indices = p["pairs"]
        self._solver = tc.solver(self.device)
        self._has_scales = False
        self._has_warp = False
        self._depth_orig = initial_depth_dir is not None
        if not p["color_frames"]:
            raise ValueError(f"{path}: no flow pair survives: the dataset is empty")
        first = load_color(self.color_fmt.format(p["color_frames"][0]))
        if first.ndim != 3 or first.shape[2] != 3:
            raise ValueError(f"receive image of shape {first.shape} whose #channels != 3")
        self.height, self.width = first.shape[:2]
        # the store holds frames [0, F): every frame a sample names, and what update_poses fills
        self._F = max(max(p["color_frames"]) + 1, self.num_frames)
        s = self._solver
        s.dataset_create(self._F, self.height, self.width, p["directed"], p["pairs"], self.use_temporal_smooth_loss,
                         self._depth_orig, self.num_frames)
        npx = self.height * self.width
        self._upload_runs(p["color_frames"], max(1, CHUNK_BYTES // (12 * npx)),
                          lambda ks: s.dataset_set_colors(ks[0], np.stack([load_color(self.color_fmt.format(k)) for k in ks])))
        per = max(1, CHUNK_BYTES // (9 * npx))
        for q0 in range(0, len(p["directed"]), per):
            part = p["directed"][q0:q0 + per]
            s.dataset_set_flows(q0, np.stack([load_flow(self.flow_fmt.format(a, b)) for a, b in part]),
                                np.stack([load_mask(self.mask_fmt.format(a, b)) for a, b in part]))
        if self._depth_orig:
            fmt = pjoin(initial_depth_dir, "frame_{:06d}.raw")
            pair_frames = sorted({k for pair in p["pairs"] for k in pair})

            def depth_of(k):
                with np.errstate(divide="ignore"):
                    return (1.0 / dataset_io.read_raw_image(fmt.format(k))).astype(np.float32)
            self._upload_runs(pair_frames, max(1, CHUNK_BYTES // (4 * npx)),
                              lambda ks: s.dataset_set_depth_orig(ks[0], np.stack([depth_of(k) for k in ks])))
        if meta_file is not None:
            with open(meta_file, "rb") as f:
                meta = np.load(f)
                ext = np.asarray(meta["extrinsics"], np.float32)
                intr = np.asarray(meta["intrinsics"], np.float32)
            assert ext.shape[0] == intr.shape[0], "#extrinsics({}) != #intrinsics({})".format(ext.shape[0], intr.shape[0])
            self._set_cameras(ext, intr)

    @staticmethod
    def _upload_runs(keys, per, upload):
        """upload(ks) for runs ks of consecutive keys, at most `per` long"""
        run = []
        for k in keys:
            if run and (k != run[-1] + 1 or len(run) == per):
                upload(run)
                run = []
            run.append(k)
        if run:
            upload(run)

    def _set_cameras(self, ext, intr):
        """cameras of frames [0, len(ext)) into the store's [0, F) (frames beyond either stay zero)"""
        e = np.zeros((self._F, 3, 4), np.float32)
        i = np.zeros((self._F, 4), np.float32)
        n = min(self._F, ext.shape[0])
        e[:n], i[:n] = ext[:n], intr[:n]
        self._solver.dataset_set_cameras(e, i)

    def update_poses(self, depth_video, host_maps=False):
        """Update extrinsics, intrinsics, depth and spatial transformation from a depth_video.  This should be called after every
        pose optimization (reference loaders/video_dataset.py:153-217)."""
        ds = depth_video.depthStream(depth_video.numDepthStreams() - 1)
        ext, intr = cameras_of(depth_video, self.frames)
        f0 = ds.frame(self.frames[0])
        dd, sd = f0.depthXform().desc(), f0.spatialXform().desc()
        # We only support scale-based transforms at the moment.
        assert dd.depthType.name == "Identity" or dd.valueXform.name == "Scale"
        if dd.depthType.name not in ("Identity", "Global", "Grid"):
            raise RuntimeError(f"Unsupported depth transform type '{dd.type}'.")
        if sd.spatialType.name not in _VALID_SPATIAL:
            raise RuntimeError(f"Unsupported spatial transform type '{sd.type}'.")
        self._set_cameras(ext, intr)
        s = self._solver
        F, H, W = self._F, self.height, self.width
        depthwise = dd.depthType.name == "Grid" and int(list(dd.gridSize)[2]) > 1
        if host_maps or depthwise:
            # the reference's path: one paramMap and one warp per frame on the host
            is_map = dd.depthType.name == "Grid"
            scales = np.zeros((F, H, W) if is_map else (F,), np.float32)
            warp = np.zeros((F, 2, H, W), np.float32)
            for i in self.frames:
                f = ds.frame(i)
                if dd.depthType.name == "Identity":
                    scales[i] = 1.0
                elif dd.depthType.name == "Global":
                    scales[i] = f.depthXform().params()[0]
                else:
                    scales[i] = np.asarray(f.depthXform().paramMap(f))
                warp[i] = np.transpose(np.asarray(f.spatialXform().warp(ds.height(), ds.width()), np.float32), (2, 0, 1))
            s.dataset_set_maps(scales, warp)
        else:
            def params_of(get):
                rows = {i: np.asarray(get(ds.frame(i)).params(), np.float64).reshape(-1) for i in self.frames}
                out = np.zeros((F, max(r.size for r in rows.values())), np.float64)
                for i, r in rows.items():
                    out[i, :r.size] = r
                return out
            s.dataset_set_xforms(_xform_desc(dd), params_of(lambda f: f.depthXform()), _xform_desc(sd),
                                 params_of(lambda f: f.spatialXform()))
        self._has_scales = True
        self._has_warp = True

    def __len__(self):
        return len(self.flow_indices)

    def batch(self, indices):
        """(images, metadata) of the samples `indices` (a list, a CPU tensor or a tensor on the device), as tensors on the device:
        one kernel launch on torch's current stream, no host synchronisation.  Host indices are checked here; a device tensor's
        cannot be (the kernel clamps and counts them, api.Solver.dataset_bad_indices)."""
        import ctypes as C

        import torch
        from . import api
        if torch.is_tensor(indices) and indices.is_cuda:
            idx = indices.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        else:
            host = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
            if host.numel() and (int(host.min()) < 0 or int(host.max()) >= len(self)):
                raise IndexError(f"VideoDataset: index out of range in {host.tolist()} ({len(self)} samples)")
            idx = host.to(self.device)
        B = idx.numel()
        if B == 0:
            raise ValueError("VideoDataset: empty batch")
        want_warp = self.recon != "colmap"
        if want_warp and not self._has_warp:
            raise RuntimeError("VideoDataset: no warp table (call update_poses first; recon='colmap' needs none)")
        s = self._solver
        info = s._dataset_info()
        shapes = api.dataset_batch_shapes(B, 6 if self.use_temporal_smooth_loss else 2, self.height, self.width,
                                          info["scale_mode"] if self._has_scales else 0, want_warp, self._depth_orig)
        with torch.cuda.device(self.device):
            flat = {k: torch.empty(shape, dtype=getattr(torch, dtype), device=self.device) for k, (shape, dtype) in shapes.items()}
            out = api.dataset_batch_out({k: t.data_ptr() for k, t in flat.items()})
            stream = torch.cuda.current_stream().cuda_stream
            s._check(s._fn("dataset_batch_device")(s._h, C.c_int32(B), C.c_void_p(idx.data_ptr()), C.byref(out), C.c_void_p(stream)))
        return api.nest_batch(flat)

    def __getitem__(self, index):
        """One sample with the reference's per-sample shapes (no batch dimension), as device tensors."""
        images, meta = self.batch([int(index)])

        def first(v):
            if isinstance(v, dict):
                return {k: first(x) for k, x in v.items()}
            if isinstance(v, list):
                return [first(x) for x in v]
            return v[0]
        return images[0], first(meta)

    def loader(self, batch_size, shuffle=False, generator=None, drop_last=False):
        """Iterates over one epoch of batches (replaces torch.utils.data.DataLoader(dataset, batch_size, shuffle, ...) and
        to_device).  shuffle draws torch.randperm(len(dataset)) on the device, from `generator` (a torch.Generator of the
        device) when given."""
        import torch
        n = len(self)
        if shuffle:
            order = torch.randperm(n, device=self.device, generator=generator)
        else:
            order = torch.arange(n, device=self.device)
        for i in range(0, n, batch_size):
            part = order[i:i + batch_size]
            if drop_last and part.numel() < batch_size:
                return
            yield self.batch(part)
