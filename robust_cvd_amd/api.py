"""Python host mirror of the optimizer path over the C ABI of libcvd_hip.so (include/cvd_hip.h).

`Solver` has the method surface of the reference's DepthVideoProcessor / DepthVideoPoseOptimizer calls used by
`pose_optimization.py` (reference pose_optimization.py:177-240): reset_depth_xforms, reset_spatial_xforms,
normalize_depth, pose_optimization (= optimizePoses), grid_xform_split.  There is NO fallback: if the HIP
library is missing, or no GPU is usable, construction raises.
"""
import collections
import ctypes as C
import os
import sys

from . import build as _build
from .binding import Binding
from .ctypes_types import OptParams, SolveSummary, XformDesc  # noqa: F401 (re-exported)

_lib = None
_variant = None


class SolverOptions(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint64),
        ("pcg_relative_tolerance", C.c_double),
        ("pcg_max_iterations", C.c_int32),
        ("verbose", C.c_int32),
        ("coarse_level", C.c_int32),
        ("robust_loss", C.c_int32),
        ("dense_matrix_free", C.c_int32),
        ("block_inverse_variant", C.c_int32),
        ("coarse_dense_max_unknowns", C.c_int32),
        ("coarse_rebuild_excess", C.c_int32),
        ("coarse_update_budget", C.c_int64),
        ("coarse_dense_shift", C.c_double),
        ("constraint_order", C.c_int32),
        ("coarse_rebuild_excess_dense", C.c_int32),
        ("pcg_fused_tail", C.c_int32),
        ("coarse_dense_row_split", C.c_int32),
        ("dist_owner_update", C.c_int32),
        ("temporal_level", C.c_int32),
        ("temporal_step", C.c_int32),
        ("temporal_grid_x", C.c_int32),
        ("temporal_grid_y", C.c_int32),
        ("coarse_temporal_step", C.c_int32),
        ("coarse_over_budget", C.c_int32),
        ("coarse_temporal_min_frames", C.c_int32),
        ("temporal_weight", C.c_double),
    ]


class DebugOptions(C.Structure):
    """include/cvd_hip_debug.h cvd_debug_options: test / measurement hooks, not part of the product interface."""
    _fields_ = [
        ("struct_size", C.c_uint64),
        ("force_iterations", C.c_int32),
        ("force_sharded_path", C.c_int32),
        ("pcg_lockstep", C.c_int32),
        ("stall_fused_tail_once", C.c_int32),
        ("tail_no_row_staging", C.c_int32),
        ("tail_closes_scalars", C.c_int32),
        ("asm_force_stage_depth", C.c_int32),
        ("asm_force_part_units", C.c_int32),
    ]


class ConsistencyDesc(C.Structure):
    """include/cvd_hip.h cvd_consistency_desc"""
    _fields_ = [
        ("struct_size", C.c_uint64),
        ("precision", C.c_int32),
        ("num_frames", C.c_int32),
        ("num_pairs", C.c_int32),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("distance_type", C.c_int32),
        ("have_warp", C.c_int32),
        ("reserved", C.c_int32),
        ("lambda_reprojection", C.c_double),
        ("lambda_disparity", C.c_double),
        ("lambda_depth_ratio", C.c_double),
        ("distance_scale", C.c_double),
        ("distance_alpha", C.c_double),
    ]


class SceneFlowDesc(C.Structure):
    """include/cvd_hip.h cvd_scene_flow_desc"""
    _fields_ = [
        ("struct_size", C.c_uint64),
        ("precision", C.c_int32),
        ("num_frames", C.c_int32),
        ("num_pairs", C.c_int32),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("distance_type_static", C.c_int32),
        ("distance_type_smooth", C.c_int32),
        ("have_warp", C.c_int32),
        ("lambda_static", C.c_double),
        ("lambda_smooth_reprojection", C.c_double),
        ("lambda_smooth_disparity", C.c_double),
        ("lambda_smooth_depth_ratio", C.c_double),
        ("distance_scale", C.c_double),
        ("distance_alpha", C.c_double),
    ]


class SpatialDesc(C.Structure):
    """include/cvd_hip.h cvd_spatial_desc"""
    _fields_ = [
        ("struct_size", C.c_uint64),
        ("precision", C.c_int32),
        ("num_frames", C.c_int32),
        ("frames_per_sample", C.c_int32),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("reserved", C.c_int32),
        ("lambda_disparity_smooth", C.c_double),
        ("sigma_color_grad", C.c_double),
        ("lambda_contrast_loss", C.c_double),
        ("contrast_thresh", C.c_double),
    ]


class ParamDesc(C.Structure):
    """include/cvd_hip.h cvd_param_desc"""
    _fields_ = [
        ("struct_size", C.c_uint64),
        ("precision", C.c_int32),
        ("num_tensors", C.c_int32),
    ]


class ParamRecord(C.Structure):
    """include/cvd_hip.h cvd_param_record"""
    _fields_ = [
        ("beta1", C.c_double),
        ("beta2", C.c_double),
        ("eps", C.c_double),
        ("grad_decay", C.c_double),
        ("param_decay", C.c_double),
        ("step", C.c_double),
        ("denom_scale", C.c_double),
        ("rule", C.c_int32),
        ("reserved", C.c_int32),
    ]


class DatasetDesc(C.Structure):
    """include/cvd_hip.h cvd_dataset_desc"""
    _fields_ = [
        ("struct_size", C.c_uint64),
        ("num_frames", C.c_int32),
        ("height", C.c_int32),
        ("width", C.c_int32),
        ("num_pairs", C.c_int32),
        ("num_samples", C.c_int32),
        ("temporal", C.c_int32),
        ("has_depth_orig", C.c_int32),
        ("neighbor_rule_frames", C.c_int32),
    ]


class DatasetBatchOut(C.Structure):
    """include/cvd_hip.h cvd_dataset_batch_out: addresses of a batch's tensors (host or device, as the entry point says)"""
    _fields_ = [
        ("struct_size", C.c_uint64),
        ("images", C.c_void_p),
        ("extrinsics", C.c_void_p),
        ("intrinsics", C.c_void_p),
        ("gc_indices", C.c_void_p),
        ("gc_flows", C.c_void_p * 2),
        ("gc_masks", C.c_void_p * 2),
        ("ts_indices", C.c_void_p),
        ("ts_flows", C.c_void_p * 4),
        ("ts_masks", C.c_void_p * 4),
        ("ts_valid", C.c_void_p),
        ("scales", C.c_void_p),
        ("warp", C.c_void_p),
        ("depth_orig", C.c_void_p),
    ]


PARAM_RULES = {"adam": 0, "radam": 1, "radam_sgd": 2, "moments": 3}  # include/cvd_hip.h CVD_PARAM_RULE_*

DISTANCE_TYPES = {"l1": 0, "l2": 1, "smooth_l1": 2, "cauchy": 3, "general": 4}  # include/cvd_hip.h CVD_DISTANCE_*
CONSISTENCY_TERMS = ("reproj", "disp", "depth ratio")   # the keys of the reference's batch_losses, in the order of terms[P][3]
# the keys of the reference's SceneFlowLoss batch_losses, in the order of terms[P][4]
SCENE_FLOW_TERMS = ("static", "smooth_reproj", "smooth_disparity", "smooth_depth_ratio")

ABI_REVISION = 6  # include/cvd_hip.h: CVD_ABI_REVISION


def consistency_desc(precision, num_frames, num_pairs, height, width, distance="l1", scale=1.0, alpha=1.0,
                     lambdas=(1.0, 0.0, 100.0), have_warp=False):
    """A stamped cvd_consistency_desc; precision: 0 / numpy float32 = f32, 1 / float64 = f64."""
    if distance not in DISTANCE_TYPES:
        raise ValueError(f"unknown distance {distance!r} (one of {sorted(DISTANCE_TYPES)})")
    d = ConsistencyDesc()
    d.struct_size = C.sizeof(ConsistencyDesc) | (ABI_REVISION << 32)
    d.precision = int(precision)
    d.num_frames, d.num_pairs, d.height, d.width = int(num_frames), int(num_pairs), int(height), int(width)
    d.distance_type = DISTANCE_TYPES[distance]
    d.have_warp = int(bool(have_warp))
    d.lambda_reprojection, d.lambda_disparity, d.lambda_depth_ratio = (float(v) for v in lambdas)
    d.distance_scale, d.distance_alpha = float(scale), float(alpha)
    return d


def scene_flow_desc(precision, num_frames, num_pairs, height, width, distance_static="l1", distance_smooth="l1", scale=1.0,
                    alpha=1.0, lambdas=(1.0, 1.0, 0.0, 100.0), have_warp=False):
    """A stamped cvd_scene_flow_desc; lambdas = (static, smooth reprojection, smooth disparity, smooth depth ratio)."""
    for distance in (distance_static, distance_smooth):
        if distance not in DISTANCE_TYPES:
            raise ValueError(f"unknown distance {distance!r} (one of {sorted(DISTANCE_TYPES)})")
    d = SceneFlowDesc()
    d.struct_size = C.sizeof(SceneFlowDesc) | (ABI_REVISION << 32)
    d.precision = int(precision)
    d.num_frames, d.num_pairs, d.height, d.width = int(num_frames), int(num_pairs), int(height), int(width)
    d.distance_type_static, d.distance_type_smooth = DISTANCE_TYPES[distance_static], DISTANCE_TYPES[distance_smooth]
    d.have_warp = int(bool(have_warp))
    (d.lambda_static, d.lambda_smooth_reprojection, d.lambda_smooth_disparity,
     d.lambda_smooth_depth_ratio) = (float(v) for v in lambdas)
    d.distance_scale, d.distance_alpha = float(scale), float(alpha)
    return d


def spatial_desc(precision, num_frames, frames_per_sample, height, width, lambda_disparity_smooth=0.0, sigma_color_grad=1.0,
                 lambda_contrast_loss=0.0, contrast_thresh=1.05):
    """A stamped cvd_spatial_desc; precision: 0 / numpy float32 = f32, 1 / float64 = f64."""
    d = SpatialDesc()
    d.struct_size = C.sizeof(SpatialDesc) | (ABI_REVISION << 32)
    d.precision = int(precision)
    d.num_frames, d.frames_per_sample, d.height, d.width = int(num_frames), int(frames_per_sample), int(height), int(width)
    d.lambda_disparity_smooth, d.sigma_color_grad = float(lambda_disparity_smooth), float(sigma_color_grad)
    d.lambda_contrast_loss, d.contrast_thresh = float(lambda_contrast_loss), float(contrast_thresh)
    return d


def param_desc(precision, num_tensors):
    """A stamped cvd_param_desc; precision: 0 / numpy float32 = f32, 1 / float64 = f64."""
    d = ParamDesc()
    d.struct_size = C.sizeof(ParamDesc) | (ABI_REVISION << 32)
    d.precision, d.num_tensors = int(precision), int(num_tensors)
    return d


def dataset_desc(num_frames, height, width, num_pairs, num_samples, temporal, has_depth_orig=False, neighbor_rule_frames=0):
    """A stamped cvd_dataset_desc."""
    d = DatasetDesc()
    d.struct_size = C.sizeof(DatasetDesc) | (ABI_REVISION << 32)
    d.num_frames, d.height, d.width = int(num_frames), int(height), int(width)
    d.num_pairs, d.num_samples = int(num_pairs), int(num_samples)
    d.temporal, d.has_depth_orig = int(bool(temporal)), int(bool(has_depth_orig))
    d.neighbor_rule_frames = int(neighbor_rule_frames)
    return d


def dataset_batch_shapes(B, N, H, W, scale_mode=0, warp=False, depth_orig=False):
    """{name: (shape, dtype name)} of the tensors of a batch of B samples, in the order of cvd_dataset_batch_out; the lists
    gc_flows .. ts_masks are named `gc_flows0` ...  scale_mode: 0 no scales, 1 scalars (B, N, 1, 1), 2 maps (B, N, H, W)."""
    out = {"images": ((B, N, 3, H, W), "float32"), "extrinsics": ((B, N, 3, 4), "float32"), "intrinsics": ((B, N, 4), "float32"),
           "gc_indices": ((B, 2), "int64")}
    out.update({f"gc_flows{d}": ((B, 2, H, W), "float32") for d in range(2)})
    out.update({f"gc_masks{d}": ((B, 1, H, W), "float32") for d in range(2)})
    if N > 2:
        out["ts_indices"] = ((B, 4), "int64")
        out.update({f"ts_flows{d}": ((B, 2, H, W), "float32") for d in range(4)})
        out.update({f"ts_masks{d}": ((B, 1, H, W), "float32") for d in range(4)})
        out["ts_valid"] = ((B, 2, 1), "float32")
    if scale_mode:
        out["scales"] = ((B, N, H, W) if scale_mode == 2 else (B, N, 1, 1), "float32")
    if warp:
        out["warp"] = ((B, N, 2, H, W), "float32")
    if depth_orig:
        out["depth_orig"] = ((B, 2, H, W), "float32")
    return out


def dataset_batch_out(addresses):
    """A stamped cvd_dataset_batch_out from {name of dataset_batch_shapes: address}."""
    o = DatasetBatchOut()
    o.struct_size = C.sizeof(DatasetBatchOut) | (ABI_REVISION << 32)
    for name, a in addresses.items():
        if name[-1].isdigit():
            getattr(o, name[:-1])[int(name[-1])] = a
        else:
            setattr(o, name, a)
    return o


def nest_batch(flat):
    """The flat tensors of dataset_batch_shapes as (images, metadata) with the nesting and key names of the reference's
    VideoDataset (loaders/video_dataset.py:330-398)."""
    meta = {"extrinsics": flat["extrinsics"], "intrinsics": flat["intrinsics"],
            "geometry_consistency": {"indices": flat["gc_indices"], "flows": [flat["gc_flows0"], flat["gc_flows1"]],
                                     "masks": [flat["gc_masks0"], flat["gc_masks1"]]}}
    if "ts_indices" in flat:
        meta["temporal_smoothness"] = {"indices": flat["ts_indices"], "flows": [flat[f"ts_flows{d}"] for d in range(4)],
                                       "masks": [flat[f"ts_masks{d}"] for d in range(4)], "valid": flat["ts_valid"]}
    for k in ("scales", "warp", "depth_orig"):
        if k in flat:
            meta[k] = flat[k]
    return flat["images"], meta


_hip = None


def _hip_runtime():
    """The HIP runtime this process already holds (libcvd_hip.so's dependency), for the few raw device buffers the numpy mirror
    of a `*_device` entry point needs (Solver.dataset_batch(device_entry=True)); torch callers use torch's tensors instead."""
    global _hip
    if _hip is None:
        # The runtime libcvd_hip.so itself is bound to: symbols looked up through the library's own handle resolve in its
        # dependencies.  (A process may hold a second copy -- torch imported after the library brings its own -- and device memory
        # of one runtime means nothing to the other.)
        lib = C.CDLL(load_library()._name)
        if not hasattr(lib, "hipMalloc"):
            raise RuntimeError("the HIP runtime is not loaded in this process")
        lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        lib.hipFree.argtypes = [C.c_void_p]
        lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip = lib
    return _hip


RAFT_MAX_LEVELS = 4   # kRaftMaxLevels / kRaftMaxRadius of csrc/cvd_raftops.h
RAFT_MAX_RADIUS = 4


def raft_level_shapes(h2, w2, levels):
    """The (height, width) of the `levels` correlation maps over an h2 x w2 frame: each floor(half) of the one above.  ValueError
    (before any device work) outside the operators' domain: 1..4 levels, the coarsest at least 2 x 2 -- the reference's sampler
    divides by (size - 1), a 1-wide level is NaN there."""
    if not 1 <= int(levels) <= RAFT_MAX_LEVELS:
        raise ValueError(f"RAFT correlation: num_levels must be 1..{RAFT_MAX_LEVELS} (got {levels})")
    shapes = [(int(h2) >> l, int(w2) >> l) for l in range(int(levels))]
    if min(shapes[-1]) < 2:
        raise ValueError(f"RAFT correlation: level {levels - 1} of a {h2} x {w2} map is {shapes[-1][0]} x {shapes[-1][1]}, below "
                         "2 x 2 (the reference's lookup is NaN there)")
    return shapes


def raft_check_radius(radius):
    if not 1 <= int(radius) <= RAFT_MAX_RADIUS:
        raise ValueError(f"RAFT correlation: radius must be 1..{RAFT_MAX_RADIUS} (got {radius})")
    return int(radius)


def raft_check_dim(dim):
    if int(dim) < 1:
        raise ValueError(f"RAFT correlation: dim must be >= 1 (got {dim})")
    return int(dim)


def raft_check_upsample(flow_shape, mask_shape):
    """(N, H, W) of flow [N, 2, H, W] and mask [N, 576, H, W]; ValueError for anything else."""
    if len(flow_shape) != 4 or flow_shape[1] != 2 or min(flow_shape) < 1:
        raise ValueError(f"RAFT upsampling: flow must be (N, 2, H, W) (got {tuple(flow_shape)})")
    N, _, H, W = (int(v) for v in flow_shape)
    if tuple(mask_shape) != (N, 576, H, W):
        raise ValueError(f"RAFT upsampling: mask must be {(N, 576, H, W)} (got {tuple(mask_shape)})")
    return N, H, W


GRU_HIDDEN = 128     # kGruHidden / kGruInput / kGruBlockChannels / kGruMaxSegments of csrc/cvd_raftgru.h
GRU_INPUT = 256
GRU_SEGMENT_MULTIPLE = 32
GRU_MAX_SEGMENTS = 3
GRU_PARAMETERS = ("convz1", "convr1", "convq1", "convz2", "convr2", "convq2")    # the entry point's order


def raft_gru_weight_shape(name):
    """Shape of `<name>.weight` of the reference's SepConvGRU(128, 256): 1 x 5 for the first half, 5 x 1 for the second."""
    return (GRU_HIDDEN, GRU_HIDDEN + GRU_INPUT) + ((1, 5) if name.endswith("1") else (5, 1))


def raft_check_gru(h_shape, x_shapes, weight_shapes, bias_shapes):
    """(B, H, W) of h [B, 128, H, W] and the segments of x, each [B, C_i, H, W] with C_i a multiple of 32 and sum 256; the six
    weight and six bias shapes in GRU_PARAMETERS order.  ValueError (before any device work) for anything else."""
    who = "RAFT SepConvGRU"
    h_shape = tuple(int(v) for v in h_shape)
    if len(h_shape) != 4 or h_shape[1] != GRU_HIDDEN:
        raise ValueError(f"{who}: h must be (B, {GRU_HIDDEN}, H, W) (got {h_shape}); hidden_dim is fixed at {GRU_HIDDEN}")
    B, _, H, W = h_shape
    if B * H * W == 0:
        raise ValueError(f"{who}: B H W = 0 (h is {h_shape})")
    x_shapes = [tuple(int(v) for v in s) for s in x_shapes]
    if not 1 <= len(x_shapes) <= GRU_MAX_SEGMENTS:
        raise ValueError(f"{who}: x must be one tensor or a tuple of up to {GRU_MAX_SEGMENTS} (got {len(x_shapes)})")
    for s in x_shapes:
        if len(s) != 4 or (s[0], s[2], s[3]) != (B, H, W):
            raise ValueError(f"{who}: a segment of x has shape {s}, expected ({B}, C, {H}, {W})")
        if s[1] < GRU_SEGMENT_MULTIPLE or s[1] % GRU_SEGMENT_MULTIPLE:
            raise ValueError(f"{who}: a segment of x has {s[1]} channels, not a positive multiple of {GRU_SEGMENT_MULTIPLE}")
    if sum(s[1] for s in x_shapes) != GRU_INPUT:
        raise ValueError(f"{who}: x has {sum(s[1] for s in x_shapes)} channels; input_dim is fixed at {GRU_INPUT}")
    if len(weight_shapes) != 6 or len(bias_shapes) != 6:
        raise ValueError(f"{who}: six weights and six biases are expected, in the order {GRU_PARAMETERS}")
    for name, ws, bs in zip(GRU_PARAMETERS, weight_shapes, bias_shapes):
        if tuple(ws) != raft_gru_weight_shape(name):
            raise ValueError(f"{who}: {name}.weight must be {raft_gru_weight_shape(name)} (got {tuple(ws)})")
        if tuple(bs) != (GRU_HIDDEN,):
            raise ValueError(f"{who}: {name}.bias must be ({GRU_HIDDEN},) (got {tuple(bs)})")
    return B, H, W


CONV_KERNEL_SIZES = (1, 3, 7)     # the instantiations of csrc/cvd_raftconv.h; kConvSegmentMultiple / kConvMaxSegments / kConvTile
CONV_SEGMENT_MULTIPLE = 32
CONV_MAX_SEGMENTS = 3
CONV_STACK_MULTIPLE = 64
RAFT_COR_PLANES = 4 * 81          # corr_levels (2 corr_radius + 1)^2 of the RAFT the reference builds
# The update block's 15 convolutions in the order of cvd_raft_update_block_device's weight and bias tables (the order of the
# reference module's state dict): (name, out channels, in channels, filter size).  The six of the GRU are GRU_PARAMETERS.
UPDATE_BLOCK_PARAMETERS = ("encoder.convc1", "encoder.convc2", "encoder.convf1", "encoder.convf2", "encoder.conv",
                           "gru.convz1", "gru.convr1", "gru.convq1", "gru.convz2", "gru.convr2", "gru.convq2",
                           "flow_head.conv1", "flow_head.conv2", "mask.0", "mask.2")


def raft_block_weight_shape(name, cor_planes=RAFT_COR_PLANES):
    """Shape of `<name>.weight` of the reference's BasicUpdateBlock(hidden_dim=128, input_dim=128)."""
    if name.startswith("gru."):
        return raft_gru_weight_shape(name[4:])
    o, c, k = {"encoder.convc1": (256, int(cor_planes), 1), "encoder.convc2": (192, 256, 3), "encoder.convf1": (128, 2, 7),
               "encoder.convf2": (64, 128, 3), "encoder.conv": (126, 256, 3), "flow_head.conv1": (256, 128, 3),
               "flow_head.conv2": (2, 256, 3), "mask.0": (256, 128, 3), "mask.2": (576, 256, 1)}[name]
    return (o, c, k, k)


def raft_check_conv2d(segment_shapes, weight_shapes, bias_shapes, out_channels_total=None, out_first=0, stride=1, dilation=1,
                      groups=1):
    """(B, H, W, N) of one convolution of csrc/cvd_raftconv.h: the input's segments [B, C_i, H, W] (one of any C >= 1, or up to
    three in multiples of 32), one weight [O, sum C_i, k, k] with k in (1, 3, 7) or two alike stacked along O (O a multiple of 64),
    biases [O]; N = the output channels written, at out_first of a tensor of out_channels_total (default: exactly N).
    ValueError (before any device work) for anything else."""
    who = "RAFT conv2d"
    for name, v in (("stride", stride), ("dilation", dilation), ("groups", groups)):
        if v != 1 and tuple(v if isinstance(v, (tuple, list)) else (v,)) not in ((1,), (1, 1)):
            raise ValueError(f"{who}: {name} must be 1 (got {v})")
    segs = [tuple(int(v) for v in s) for s in segment_shapes]
    if not 1 <= len(segs) <= CONV_MAX_SEGMENTS:
        raise ValueError(f"{who}: the input must be one tensor or a tuple of up to {CONV_MAX_SEGMENTS} (got {len(segs)})")
    if len(segs[0]) != 4:
        raise ValueError(f"{who}: the input must be (B, C, H, W) (got {segs[0]})")
    B, _, H, W = segs[0]
    if B * H * W == 0:
        raise ValueError(f"{who}: B H W = 0 (the input is {segs[0]})")
    for s in segs:
        if len(s) != 4 or (s[0], s[2], s[3]) != (B, H, W):
            raise ValueError(f"{who}: a segment has shape {s}, expected ({B}, C, {H}, {W})")
        if s[1] < 1:
            raise ValueError(f"{who}: a segment has {s[1]} channels")
        if len(segs) > 1 and s[1] % CONV_SEGMENT_MULTIPLE:
            raise ValueError(f"{who}: a segment has {s[1]} channels, not a positive multiple of {CONV_SEGMENT_MULTIPLE} "
                             "(several segments)")
    cin = sum(s[1] for s in segs)
    ws = [tuple(int(v) for v in s) for s in weight_shapes]
    bs = [tuple(int(v) for v in s) for s in bias_shapes]
    if not 1 <= len(ws) <= 2 or len(bs) != len(ws):
        raise ValueError(f"{who}: one weight and bias, or two stacked, are expected (got {len(ws)}, {len(bs)})")
    if len(ws[0]) != 4 or ws[0][2] != ws[0][3] or ws[0][2] not in CONV_KERNEL_SIZES:
        raise ValueError(f"{who}: the filter must be square of size {CONV_KERNEL_SIZES} (weight {ws[0]})")
    if ws[0][0] < 1:
        raise ValueError(f"{who}: no output channels (weight {ws[0]})")
    if ws[0][1] != cin:
        raise ValueError(f"{who}: the input has {cin} channels, the weight {ws[0]} takes {ws[0][1]}")
    for w, b in zip(ws, bs):
        if w != ws[0]:
            raise ValueError(f"{who}: stacked weights must have one shape (got {ws})")
        if b != (w[0],):
            raise ValueError(f"{who}: a bias must be ({w[0]},) (got {b})")
    if len(ws) == 2 and ws[0][0] % CONV_STACK_MULTIPLE:
        raise ValueError(f"{who}: stacked weights need output channels in multiples of {CONV_STACK_MULTIPLE} (got {ws[0][0]})")
    N = ws[0][0] * len(ws)
    total = N if out_channels_total is None else int(out_channels_total)
    if int(out_first) < 0 or int(out_first) + N > total:
        raise ValueError(f"{who}: the output window, channels {out_first} .. {int(out_first) + N - 1}, exceeds the tensor's {total}")
    return B, H, W, N


def raft_check_update_block(net_shape, inp_shape, corr_shape, flow_shape, weight_shapes, bias_shapes):
    """(B, H, W) of BasicUpdateBlock.forward's inputs: net and inp [B, 128, H, W], corr [B, cor_planes, H, W] with cor_planes the
    in_channels of encoder.convc1.weight, flow [B, 2, H, W]; the 15 weight and bias shapes in UPDATE_BLOCK_PARAMETERS order.
    ValueError (before any device work) for anything else."""
    who = "RAFT update block"
    net_shape, inp_shape, corr_shape, flow_shape = (tuple(int(v) for v in s) for s in (net_shape, inp_shape, corr_shape, flow_shape))
    if len(net_shape) != 4 or net_shape[1] != GRU_HIDDEN:
        raise ValueError(f"{who}: net must be (B, {GRU_HIDDEN}, H, W) (got {net_shape})")
    B, _, H, W = net_shape
    if B * H * W == 0:
        raise ValueError(f"{who}: B H W = 0 (net is {net_shape})")
    if inp_shape != (B, 128, H, W):
        raise ValueError(f"{who}: inp must be {(B, 128, H, W)} (got {inp_shape})")
    if flow_shape != (B, 2, H, W):
        raise ValueError(f"{who}: flow must be {(B, 2, H, W)} (got {flow_shape})")
    if len(weight_shapes) != 15 or len(bias_shapes) != 15:
        raise ValueError(f"{who}: 15 weights and 15 biases are expected, in the order {UPDATE_BLOCK_PARAMETERS}")
    ws = [tuple(int(v) for v in s) for s in weight_shapes]
    if len(ws[0]) != 4 or ws[0][1] < 1:
        raise ValueError(f"{who}: encoder.convc1.weight must be (256, cor_planes, 1, 1) (got {ws[0]})")
    cor_planes = ws[0][1]
    if len(corr_shape) != 4 or (corr_shape[0], corr_shape[2], corr_shape[3]) != (B, H, W):
        raise ValueError(f"{who}: corr must be ({B}, {cor_planes}, {H}, {W}) (got {corr_shape})")
    if corr_shape[1] != cor_planes:
        raise ValueError(f"{who}: corr has {corr_shape[1]} channels, encoder.convc1 takes {cor_planes}")
    for name, w, b in zip(UPDATE_BLOCK_PARAMETERS, ws, bias_shapes):
        want = raft_block_weight_shape(name, cor_planes)
        if w != want:
            raise ValueError(f"{who}: {name}.weight must be {want} (got {w})")
        if tuple(int(v) for v in b) != (want[0],):
            raise ValueError(f"{who}: {name}.bias must be ({want[0]},) (got {tuple(b)})")
    return B, H, W


ENCODER_KERNEL_SIZES = (1, 3, 7)       # the instantiations of csrc/cvd_raftenc.h
ENCODER_STRIDES = (1, 2)
ENCODER_NORM_MODES = {"none": 0, "instance": 1, "batch": 2}      # norm_mode of cvd_raft_encoder_device
# The sixteen convolutions of the reference's BasicEncoder in the order of cvd_raft_encoder_device's weight and bias tables (the
# order of the module's state dict): name -> (out channels, in channels, filter, stride); conv2's out channels are output_dim.
ENCODER_LAYERS = (("conv1", 64, 3, 7, 2),
                  ("layer1.0.conv1", 64, 64, 3, 1), ("layer1.0.conv2", 64, 64, 3, 1),
                  ("layer1.1.conv1", 64, 64, 3, 1), ("layer1.1.conv2", 64, 64, 3, 1),
                  ("layer2.0.conv1", 96, 64, 3, 2), ("layer2.0.conv2", 96, 96, 3, 1), ("layer2.0.downsample.0", 96, 64, 1, 2),
                  ("layer2.1.conv1", 96, 96, 3, 1), ("layer2.1.conv2", 96, 96, 3, 1),
                  ("layer3.0.conv1", 128, 96, 3, 2), ("layer3.0.conv2", 128, 128, 3, 1), ("layer3.0.downsample.0", 128, 96, 1, 2),
                  ("layer3.1.conv1", 128, 128, 3, 1), ("layer3.1.conv2", 128, 128, 3, 1),
                  ("conv2", None, 128, 1, 1))
ENCODER_PARAMETERS = tuple(l[0] for l in ENCODER_LAYERS)
# The fifteen norm modules, norm i behind convolution i (layerX.0.norm3 is also registered as layerX.0.downsample.1), and the order of
# a norm's four vectors in the entry point's table (the state dict's).
ENCODER_NORMS = tuple("norm1" if n == "conv1" else n.replace("downsample.0", "norm3").replace("conv", "norm")
                      for n in ENCODER_PARAMETERS[:15])
ENCODER_NORM_VECTORS = ("weight", "bias", "running_mean", "running_var")


def raft_encoder_weight_shape(name, output_dim=256):
    """Shape of `<name>.weight` of the reference's BasicEncoder(output_dim)."""
    o, c, k, _s = dict((l[0], l[1:]) for l in ENCODER_LAYERS)[name]
    return (int(output_dim) if o is None else o, c, k, k)


def raft_encoder_out_size(size, stride=8):
    """An axis of `size` pixels after stride-2 layers of padding k // 2 that multiply to `stride`: ceil(size / stride)."""
    size = int(size)
    while stride > 1:
        size = (size - 1) // 2 + 1
        stride //= 2
    return size


def raft_check_encoder_conv(x_shape, weight_shape, bias_shape, stride=1, norm_shapes=None, eps=1e-5, residual_shape=None):
    """(B, H, W, Cin, N, k, Ho, Wo) of one convolution of csrc/cvd_raftenc.h: x [B, Cin, H, W], weight [N, Cin, k, k] with k in
    (1, 3, 7), stride 1 or 2, padding k // 2, bias [N], optionally the four [N] vectors of an eval batch norm and a residual of the
    output's shape.  ValueError (before any device work) for anything else."""
    who = "RAFT encoder conv"
    x_shape, ws, bs = (tuple(int(v) for v in s) for s in (x_shape, weight_shape, bias_shape))
    if len(x_shape) != 4:
        raise ValueError(f"{who}: x must be (B, C, H, W) (got {x_shape})")
    B, C, H, W = x_shape
    if B * C * H * W == 0:
        raise ValueError(f"{who}: B C H W = 0 (x is {x_shape})")
    if H * W > 2 ** 31 - 1:
        raise ValueError(f"{who}: {H} x {W} pixels per image exceed 2^31")
    if isinstance(stride, (tuple, list)):
        if len(set(stride)) != 1:
            raise ValueError(f"{who}: stride must be the same on both axes (got {stride})")
        stride = stride[0]
    if stride not in ENCODER_STRIDES:
        raise ValueError(f"{who}: stride must be 1 or 2 (got {stride})")
    if len(ws) != 4 or ws[2] != ws[3] or ws[2] not in ENCODER_KERNEL_SIZES:
        raise ValueError(f"{who}: the filter must be square of size {ENCODER_KERNEL_SIZES} (weight {ws})")
    if ws[0] < 1:
        raise ValueError(f"{who}: no output channels (weight {ws})")
    if ws[1] != C:
        raise ValueError(f"{who}: x has {C} channels, the weight {ws} takes {ws[1]}")
    N, k = ws[0], ws[2]
    if bs != (N,):
        raise ValueError(f"{who}: bias must be ({N},) (got {bs})")
    if norm_shapes is not None:
        shapes = [tuple(int(v) for v in s) for s in norm_shapes]
        if len(shapes) != 4 or any(s != (N,) for s in shapes):
            raise ValueError(f"{who}: the norm must be four vectors ({N},) in the order {ENCODER_NORM_VECTORS} (got {shapes})")
        if not float(eps) > 0.0:
            raise ValueError(f"{who}: eps must be > 0 (got {eps})")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if residual_shape is not None and tuple(int(v) for v in residual_shape) != (B, N, Ho, Wo):
        raise ValueError(f"{who}: residual must be {(B, N, Ho, Wo)} (got {tuple(residual_shape)})")
    return B, H, W, C, N, k, Ho, Wo


def raft_check_instance_norm(x_shape, eps=1e-5, residual_shape=None):
    """(B, C, H, W) of the instance norm of csrc/cvd_raftenc.h; ValueError for an empty tensor, planes of one element (the
    reference's own refusal), eps <= 0 or a residual of another shape."""
    who = "RAFT instance norm"
    x_shape = tuple(int(v) for v in x_shape)
    if len(x_shape) != 4:
        raise ValueError(f"{who}: x must be (B, C, H, W) (got {x_shape})")
    B, C, H, W = x_shape
    if B * C * H * W == 0:
        raise ValueError(f"{who}: B C H W = 0 (x is {x_shape})")
    if H * W < 2:
        raise ValueError(f"{who}: Expected more than 1 spatial element (x is {x_shape})")
    if H * W > 2 ** 31 - 1:
        raise ValueError(f"{who}: {H} x {W} pixels per image exceed 2^31")
    if not float(eps) > 0.0:
        raise ValueError(f"{who}: eps must be > 0 (got {eps})")
    if residual_shape is not None and tuple(int(v) for v in residual_shape) != x_shape:
        raise ValueError(f"{who}: residual must be {x_shape} (got {tuple(residual_shape)})")
    return B, C, H, W


def raft_check_encoder(image_shape, weight_shapes, bias_shapes, norm="none", norm_shapes=None, eps=1e-5):
    """(B, H, W, output_dim, norm_mode, (h, w)) of BasicEncoder.forward: images [B, 3, H, W], the 16 weight and bias shapes in
    ENCODER_PARAMETERS order, norm in ("none", "instance", "batch"), for "batch" the 15 x 4 vectors' shapes in ENCODER_NORMS order;
    (h, w) = the features' size ceil(H / 8) x ceil(W / 8).  ValueError (before any device work) for anything else."""
    who = "RAFT encoder"
    if norm not in ENCODER_NORM_MODES:
        raise ValueError(f"{who}: norm must be one of {tuple(ENCODER_NORM_MODES)} (got {norm!r}; group norm is not built)")
    image_shape = tuple(int(v) for v in image_shape)
    if len(image_shape) != 4 or image_shape[1] != 3:
        raise ValueError(f"{who}: the images must be (B, 3, H, W) (got {image_shape})")
    B, _, H, W = image_shape
    if B * H * W == 0:
        raise ValueError(f"{who}: B H W = 0 (the images are {image_shape})")
    if H * W > 2 ** 31 - 1:
        raise ValueError(f"{who}: {H} x {W} pixels per image exceed 2^31")
    if len(weight_shapes) != 16 or len(bias_shapes) != 16:
        raise ValueError(f"{who}: 16 weights and 16 biases are expected, in the order {ENCODER_PARAMETERS}")
    ws = [tuple(int(v) for v in s) for s in weight_shapes]
    if len(ws[15]) != 4 or ws[15][0] < 1:
        raise ValueError(f"{who}: conv2.weight must be (output_dim, 128, 1, 1) (got {ws[15]})")
    output_dim = ws[15][0]
    for name, w, b in zip(ENCODER_PARAMETERS, ws, bias_shapes):
        want = raft_encoder_weight_shape(name, output_dim)
        if w != want:
            raise ValueError(f"{who}: {name}.weight must be {want} (got {w})")
        if tuple(int(v) for v in b) != (want[0],):
            raise ValueError(f"{who}: {name}.bias must be ({want[0]},) (got {tuple(b)})")
    if norm != "none" and not float(eps) > 0.0:
        raise ValueError(f"{who}: eps must be > 0 (got {eps})")
    if norm == "batch":
        if norm_shapes is None or len(norm_shapes) != 15:
            raise ValueError(f"{who}: batch norm needs 15 norms of four vectors, in the order {ENCODER_NORMS}")
        for name, layer, vectors in zip(ENCODER_NORMS, ENCODER_PARAMETERS, norm_shapes):
            n = raft_encoder_weight_shape(layer)[0]
            shapes = [tuple(int(v) for v in s) for s in vectors]
            if len(shapes) != 4 or any(s != (n,) for s in shapes):
                raise ValueError(f"{who}: {name} must be four vectors ({n},) in the order {ENCODER_NORM_VECTORS} (got {shapes})")
    h, w = raft_encoder_out_size(H), raft_encoder_out_size(W)
    if norm == "instance" and h * w < 2:
        raise ValueError(f"{who}: Expected more than 1 spatial element: {H} x {W} images give {h} x {w} features under instance norm")
    return B, H, W, output_dim, ENCODER_NORM_MODES[norm], (h, w)


# ---- the decoder of MiDaS v2.1 (csrc/cvd_midas.h) ----------------------------------------------------------------
MIDAS_KERNEL_SIZES = (1, 3)            # the instantiations of csrc/cvd_midas.h
MIDAS_BACKBONE_CHANNELS = (256, 512, 1024, 2048)     # layer1 .. layer4 of the ResNeXt-101 backbone
MIDAS_HEAD_MID = 32                    # output_conv.2's channels, the head kernel's only width
MIDAS_MAX_SPLIT = 32
MIDAS_TIMED_SLOTS = 44                 # kernel_ms of cvd_midas_decoder_timed
_MIDAS_UNITS = tuple(f"refinenet{r}.resConfUnit{u}.conv{c}" for r in (4, 3, 2, 1) for u in (1, 2) for c in (1, 2))
# The 23 convolutions of the reference's MidasNet.scratch in the state dict's order; the 42 keys: a weight each, a bias for all but
# the four layerK_rn.
MIDAS_STATE_DICT_LAYERS = tuple(f"layer{k}_rn" for k in (1, 2, 3, 4)) + _MIDAS_UNITS + ("output_conv.0", "output_conv.2", "output_conv.4")
MIDAS_STATE_DICT_KEYS = tuple("scratch." + n + "." + v for n in MIDAS_STATE_DICT_LAYERS
                              for v in (("weight",) if n.endswith("_rn") else ("weight", "bias")))
# The 21 of them that run, in the order of cvd_midas_decoder_device's weight table (refinenet4.resConfUnit1 never runs: the first
# fusion block is called with one input); the bias table holds those of entries 4 .. 20.
MIDAS_PARAMETERS = tuple(n for n in MIDAS_STATE_DICT_LAYERS if not n.startswith("refinenet4.resConfUnit1."))


def midas_weight_shape(name, features=256, channels=MIDAS_BACKBONE_CHANNELS):
    """Shape of `scratch.<name>.weight` of the reference's MidasNet(features) over a backbone with `channels`."""
    features = int(features)
    if name.endswith("_rn"):
        return (features, int(channels[int(name[5]) - 1]), 3, 3)
    return {"output_conv.0": (128, features, 3, 3), "output_conv.2": (MIDAS_HEAD_MID, 128, 3, 3),
            "output_conv.4": (1, MIDAS_HEAD_MID, 1, 1)}.get(name, (features, features, 3, 3))


def midas_split(K, HW, kernel_size=3):
    """The split count S of a convolution of csrc/cvd_midas.h (midasSplit there) with K = in_channels kernel_size^2 over images of HW
    pixels: as many slices of K as bring the 64-pixel tiles of ONE image to 64 workgroups per channel tile, each slice whole chains
    (4 chunks of 72 k for 3 x 3, 8 chunks of 32 for 1 x 1), at most 32.  A function of K and HW alone: not of the batch, the output
    channels or the device."""
    chunk_k, fold = (32, 8) if int(kernel_size) == 1 else (72, 4)
    chunks = (int(K) + chunk_k - 1) // chunk_k
    chains = (chunks + fold - 1) // fold
    tiles = (int(HW) + 63) // 64
    want = max(1, min(64 // tiles, MIDAS_MAX_SPLIT, chains))
    per = (chains + want - 1) // want
    return (chains + per - 1) // per


def midas_slice_channels(in_channels, kernel_size, split):
    """The channel ranges [(c0, c1), ..] of the slices a convolution runs with under `split` (a forced split may shrink: slices are
    whole chains)."""
    cc, fold = (32, 8) if int(kernel_size) == 1 else (8, 4)
    chunks = (int(in_channels) + cc - 1) // cc
    chains = (chunks + fold - 1) // fold
    per = (chains + int(split) - 1) // int(split)
    step = per * fold * cc
    return [(c0, min(c0 + step, int(in_channels))) for c0 in range(0, int(in_channels), step)]


def _midas_shape4(who, name, shape):
    shape = tuple(int(v) for v in shape)
    if len(shape) != 4:
        raise ValueError(f"{who}: {name} must be (B, C, H, W) (got {shape})")
    B, Cn, H, W = shape
    if B * Cn * H * W == 0:
        raise ValueError(f"{who}: B C H W = 0 ({name} is {shape})")
    if H * W > 2 ** 31 - 1:
        raise ValueError(f"{who}: {H} x {W} pixels per image exceed 2^31")
    return shape


def midas_check_conv(x_shape, weight_shape, bias_shape=None, a_shape=None, b_shape=None, split=0):
    """(B, H, W, Cin, N, k) of one convolution of csrc/cvd_midas.h: x [B, Cin, H, W], weight [N, Cin, k, k] with k in (1, 3), stride
    1, padding k // 2, bias [N] or None, addends a and b of the output's shape or None, split 0 (the rule) or 1 .. the chunks of K.
    ValueError (before any device work) for anything else."""
    who = "MiDaS conv"
    B, Cn, H, W = _midas_shape4(who, "x", x_shape)
    ws = tuple(int(v) for v in weight_shape)
    if len(ws) != 4 or ws[2] != ws[3] or ws[2] not in MIDAS_KERNEL_SIZES:
        raise ValueError(f"{who}: the filter must be square of size {MIDAS_KERNEL_SIZES} (weight {ws})")
    if ws[0] < 1:
        raise ValueError(f"{who}: no output channels (weight {ws})")
    if ws[1] != Cn:
        raise ValueError(f"{who}: x has {Cn} channels, the weight {ws} takes {ws[1]}")
    N, k = ws[0], ws[2]
    if bias_shape is not None and tuple(int(v) for v in bias_shape) != (N,):
        raise ValueError(f"{who}: bias must be ({N},) (got {tuple(bias_shape)})")
    for name, s in (("a", a_shape), ("b", b_shape)):
        if s is not None and tuple(int(v) for v in s) != (B, N, H, W):
            raise ValueError(f"{who}: the addend {name} must be {(B, N, H, W)} (got {tuple(s)})")
    chunks = (Cn + (32 if k == 1 else 8) - 1) // (32 if k == 1 else 8)
    if int(split) != split or not 0 <= split <= chunks:
        raise ValueError(f"{who}: split must be 0 (the rule) or 1 .. {chunks}, the chunks of K (got {split})")
    return B, H, W, Cn, N, k


def midas_check_upsample2x(x_shape):
    """(B, C, H, W) of the bilinear x 2 upsampling; ValueError for anything but a non-empty (B, C, H, W) whose output plane stays
    below 2^31 pixels."""
    who = "MiDaS upsample2x"
    B, Cn, H, W = _midas_shape4(who, "x", x_shape)
    if 4 * H * W > 2 ** 31 - 1:
        raise ValueError(f"{who}: {2 * H} x {2 * W} output pixels per plane exceed 2^31")
    return B, Cn, H, W


def midas_check_head(x_shape, weight2_shape, bias2_shape, weight4_shape, bias4_shape):
    """(B, H, W, Cin) of the output head: x [B, Cin, H, W], output_conv.2 [32, Cin, 3, 3] and [32], output_conv.4 [1, 32, 1, 1] and
    [1]."""
    who = "MiDaS head"
    B, Cn, H, W = _midas_shape4(who, "x", x_shape)
    got = [tuple(int(v) for v in s) for s in (weight2_shape, bias2_shape, weight4_shape, bias4_shape)]
    if len(got[0]) == 4 and got[0][0] != MIDAS_HEAD_MID:
        raise ValueError(f"{who}: the middle width must be {MIDAS_HEAD_MID} (output_conv.2.weight is {got[0]})")
    want = [(MIDAS_HEAD_MID, Cn, 3, 3), (MIDAS_HEAD_MID,), (1, MIDAS_HEAD_MID, 1, 1), (1,)]
    for name, g, w in zip(("output_conv.2.weight", "output_conv.2.bias", "output_conv.4.weight", "output_conv.4.bias"), got, want):
        if g != w:
            raise ValueError(f"{who}: {name} must be {w} (got {g})")
    return B, H, W, Cn


def midas_check_decoder(map_shapes, weight_shapes, bias_shapes):
    """(B, features, channels[4], heights[4], widths[4]) of the decoder: four feature maps [B, C_k, H_k, W_k] with H_k = 2 H_{k+1}
    and W_k = 2 W_{k+1} exactly, the 21 weight and 17 bias shapes in MIDAS_PARAMETERS order.  ValueError for anything else."""
    who = "MiDaS decoder"
    if len(map_shapes) != 4:
        raise ValueError(f"{who}: four feature maps are expected (got {len(map_shapes)})")
    maps = [_midas_shape4(who, f"feature map {k + 1}", s) for k, s in enumerate(map_shapes)]
    B = maps[0][0]
    for k in range(4):
        if maps[k][0] != B:
            raise ValueError(f"{who}: feature map {k + 1} has batch {maps[k][0]}, feature map 1 has {B}")
        if k and (maps[k - 1][2], maps[k - 1][3]) != (2 * maps[k][2], 2 * maps[k][3]):
            raise ValueError(f"{who}: feature map {k} is {maps[k - 1][2]} x {maps[k - 1][3]}, not twice feature map {k + 1}'s "
                             f"{maps[k][2]} x {maps[k][3]} (image sides must be multiples of 32)")
    if 16 * maps[0][2] * maps[0][3] > 2 ** 31 - 1:
        raise ValueError(f"{who}: {4 * maps[0][2]} x {4 * maps[0][3]} output pixels per image exceed 2^31")
    if len(weight_shapes) != 21 or len(bias_shapes) != 17:
        raise ValueError(f"{who}: 21 weights and 17 biases are expected, in the order {MIDAS_PARAMETERS} (biases from entry 4 on)")
    ws = [tuple(int(v) for v in s) for s in weight_shapes]
    if len(ws[0]) != 4 or ws[0][0] < 1:
        raise ValueError(f"{who}: layer1_rn.weight must be (features, {maps[0][1]}, 3, 3) (got {ws[0]})")
    features = ws[0][0]
    channels = [m[1] for m in maps]
    for i, (name, w) in enumerate(zip(MIDAS_PARAMETERS, ws)):
        want = midas_weight_shape(name, features, channels)
        if w != want:
            raise ValueError(f"{who}: {name}.weight must be {want} (got {w})")
        if i >= 4 and tuple(int(v) for v in bias_shapes[i - 4]) != (want[0],):
            raise ValueError(f"{who}: {name}.bias must be ({want[0]},) (got {tuple(bias_shapes[i - 4])})")
    return B, features, channels, [m[2] for m in maps], [m[3] for m in maps]


# ---- backward of the decoder's layers (csrc/cvd_midas_grad.h) -----------------------------------------------------
MIDAS_WGRAD_CHAIN = 256                # pixels of one fmaf chain of the weight gradient
MIDAS_WGRAD_MAX_SPLIT = 128


def midas_wgrad_split(pixels, out_channels, columns):
    """The split count S of a weight gradient of csrc/cvd_midas_grad.h (midasWgradSplit there) over `pixels` = B H W with
    `out_channels` rows and `columns` = in_channels kernel_size^2: as many slices of the pixels as bring the 64 x 64 tiles of the
    weight tensor to 1024 workgroups, each slice whole chains of 256 pixels, at most 128.  A function of the three sizes alone."""
    tiles = ((int(out_channels) + 63) // 64) * ((int(columns) + 63) // 64)
    chains = (int(pixels) + MIDAS_WGRAD_CHAIN - 1) // MIDAS_WGRAD_CHAIN
    want = max(1, min(1024 // tiles, MIDAS_WGRAD_MAX_SPLIT, chains))
    per = (chains + want - 1) // want
    return (chains + per - 1) // per


def midas_check_conv_grad_input(gy_shape, weight_shape, add_shape=None, mask_shape=None, split=0):
    """(B, H, W, Cin, N, k) of the input gradient of one convolution: gy [B, N, H, W], weight [N, Cin, k, k] with k in (1, 3), the
    addend and the mask of gx's shape [B, Cin, H, W] or None, split 0 (the rule) or 1 .. the chunks of K = N k k.  ValueError
    (before any device work) for anything else."""
    who = "MiDaS conv grad input"
    B, N, H, W = _midas_shape4(who, "gy", gy_shape)
    ws = tuple(int(v) for v in weight_shape)
    if len(ws) != 4 or ws[2] != ws[3] or ws[2] not in MIDAS_KERNEL_SIZES:
        raise ValueError(f"{who}: the filter must be square of size {MIDAS_KERNEL_SIZES} (weight {ws})")
    if ws[0] != N:
        raise ValueError(f"{who}: gy has {N} channels, the weight {ws} gives {ws[0]}")
    if ws[1] < 1:
        raise ValueError(f"{who}: no input channels (weight {ws})")
    Cin, k = ws[1], ws[2]
    for name, s in (("addend", add_shape), ("mask", mask_shape)):
        if s is not None and tuple(int(v) for v in s) != (B, Cin, H, W):
            raise ValueError(f"{who}: the {name} must be {(B, Cin, H, W)} (got {tuple(s)})")
    chunks = (N + (32 if k == 1 else 8) - 1) // (32 if k == 1 else 8)
    if int(split) != split or not 0 <= split <= chunks:
        raise ValueError(f"{who}: split must be 0 (the rule) or 1 .. {chunks}, the chunks of K (got {split})")
    return B, H, W, Cin, N, k


def midas_check_conv_grad_weight(gy_shape, x_shape, kernel_size, split=0):
    """(B, H, W, Cin, N, k) of the weight gradient of one convolution: gy [B, N, H, W], x [B, Cin, H, W], k in (1, 3), split 0 (the
    rule) or 1 .. 128 (a forced split shrinks to whole chains of 256 pixels).  ValueError for anything else."""
    who = "MiDaS conv grad weight"
    B, N, H, W = _midas_shape4(who, "gy", gy_shape)
    B2, Cin, H2, W2 = _midas_shape4(who, "x", x_shape)
    if (B2, H2, W2) != (B, H, W):
        raise ValueError(f"{who}: gy {tuple(gy_shape)} and x {tuple(x_shape)} differ in batch or size")
    if kernel_size not in MIDAS_KERNEL_SIZES:
        raise ValueError(f"{who}: the filter must be square of size {MIDAS_KERNEL_SIZES} (got {kernel_size})")
    if int(split) != split or not 0 <= split <= MIDAS_WGRAD_MAX_SPLIT:
        raise ValueError(f"{who}: split must be 0 (the rule) or 1 .. {MIDAS_WGRAD_MAX_SPLIT} (got {split})")
    return B, H, W, Cin, N, int(kernel_size)


def midas_check_upsample2x_grad(gy_shape):
    """(B, C, H, W) of the INPUT of the upsampling whose output gradient is gy [B, C, 2 H, 2 W]."""
    who = "MiDaS upsample2x grad"
    B, Cn, Ho, Wo = _midas_shape4(who, "gy", gy_shape)
    if Ho % 2 or Wo % 2:
        raise ValueError(f"{who}: gy must be (B, C, 2 H, 2 W) (got {tuple(gy_shape)})")
    if Ho * Wo > 2 ** 31 - 1:
        raise ValueError(f"{who}: {Ho} x {Wo} output pixels per plane exceed 2^31")
    return B, Cn, Ho // 2, Wo // 2


MIDAS_SAVED = 16                       # tensors of cvd_midas_decoder_train_device's table
MIDAS_BACKWARD_SLOTS = 48              # kernel_ms of cvd_midas_decoder_backward_timed


def midas_saved_shapes(batch, features, heights, widths):
    """The 16 shapes of the table cvd_midas_decoder_train_device fills, for feature maps of `heights` x `widths` (layer1 first): the
    four layerK_rn results; refinenet4.resConfUnit2.conv1's result; for refinenet3, 2, 1 each resConfUnit1.conv1's result, the fusion
    sum and resConfUnit2.conv1's result; output_conv.0's input and its result (the head's input is recomputed from it)."""
    B, F = int(batch), int(features)
    level = [(B, F, int(h), int(w)) for h, w in zip(heights, widths)]
    twice = (2 * int(heights[0]), 2 * int(widths[0]))
    return level + [level[3]] + [level[k] for k in (2, 1, 0) for _ in range(3)] + [(B, F) + twice, (B, 128) + twice]


def midas_backward_stages(with_maps=True):
    """Names of the operator calls cvd_midas_decoder_backward_device makes, in the order of cvd_midas_decoder_backward_timed's
    kernel_ms: `<layer>:wgrad` / `<layer>:dgrad` / upsamplings / the head."""
    P = MIDAS_PARAMETERS
    out = ["output_conv.1:upsample (recomputed)", "head:backward", "output_conv.1:upsample_grad", P[18] + ":wgrad", P[18] + ":dgrad"]
    for k in range(4):
        w0 = 4 if k == 3 else 6 + 4 * (2 - k)
        u2 = w0 if k == 3 else w0 + 2
        out += [f"refinenet{k + 1}:upsample_grad", P[u2 + 1] + ":wgrad", P[u2 + 1] + ":dgrad", P[u2] + ":wgrad", P[u2] + ":dgrad"]
        if k < 3:
            out += [P[w0 + 1] + ":wgrad", P[w0 + 1] + ":dgrad", P[w0] + ":wgrad", P[w0] + ":dgrad"]
        out += [P[k] + ":wgrad"] + ([P[k] + ":dgrad"] if with_maps else [])
    return out


# ---- the ResNeXt backbone of MiDaS v2.1 (csrc/cvd_resnext.h) -----------------------------------------------------
RESNEXT_GROUP_WIDTHS = (8, 16, 32, 64)         # channels per group the grouped kernel is built for
RESNEXT_DENSE_KERNELS = ((1, 1), (1, 2), (7, 2))       # (kernel_size, stride) of the dense kernel's instantiations
RESNEXT_MAX_SPLIT = 32
RESNEXT101_32X8D = ((3, 4, 23, 3), 32, 8)      # blocks, groups, width_per_group of the reference's backbone
RESNEXT_NORM_VECTORS = ("weight", "bias", "running_mean", "running_var")       # the order of a convolution's norm table
RESNEXT_EPS = 1e-5

RxConv = collections.namedtuple("RxConv", "name norm key norm_key weight_shape in_channels out_channels kernel_size stride groups")


def resnext_conv_table(blocks=RESNEXT101_32X8D[0], groups=RESNEXT101_32X8D[1], width_per_group=RESNEXT101_32X8D[2]):
    """The convolutions of torchvision's ResNet(Bottleneck, blocks, groups=groups, width_per_group=width_per_group) in the state dict's
    order -- the stem, then per block conv1, conv2, conv3 and, in a stage's first block, downsample.0 --, the order of
    cvd_midas_backbone_device's weight and norm tables.  Per convolution: torchvision's module names of the convolution and its
    batch norm (`name`, `norm`), the same two under the reference's MidasNet.pretrained (`key`, `norm_key`: blocks.py:22-31 puts the
    stem into layer1 as a Sequential), the weight's shape, channels, filter, stride and groups."""
    blocks = tuple(int(b) for b in blocks)
    groups, width_per_group = int(groups), int(width_per_group)
    if len(blocks) != 4 or min(blocks) < 1:
        raise ValueError(f"ResNeXt: blocks must be four counts >= 1 (got {blocks})")
    if groups < 1 or width_per_group < 1:
        raise ValueError(f"ResNeXt: groups and width_per_group must be >= 1 (got {groups}, {width_per_group})")
    table = [RxConv("conv1", "bn1", "layer1.0", "layer1.1", (64, 3, 7, 7), 3, 64, 7, 2, 1)]
    cin = 64
    for k, count in enumerate(blocks):
        planes = 64 << k
        per = planes * width_per_group // 64
        width, out = per * groups, 4 * planes
        for i in range(count):
            stride = 2 if (i == 0 and k > 0) else 1
            tv = f"layer{k + 1}.{i}."
            md = f"layer1.4.{i}." if k == 0 else tv
            table.append(RxConv(tv + "conv1", tv + "bn1", md + "conv1", md + "bn1", (width, cin, 1, 1), cin, width, 1, 1, 1))
            table.append(RxConv(tv + "conv2", tv + "bn2", md + "conv2", md + "bn2", (width, per, 3, 3), width, width, 3, stride, groups))
            table.append(RxConv(tv + "conv3", tv + "bn3", md + "conv3", md + "bn3", (out, width, 1, 1), width, out, 1, 1, 1))
            if i == 0:
                table.append(RxConv(tv + "downsample.0", tv + "downsample.1", md + "downsample.0", md + "downsample.1", (out, cin, 1, 1),
                                    cin, out, 1, stride, 1))
            cin = out
    return table


def resnext_state_dict_keys(blocks=RESNEXT101_32X8D[0], groups=RESNEXT101_32X8D[1], width_per_group=RESNEXT101_32X8D[2],
                            prefix="pretrained."):
    """The backbone's state-dict keys under the reference's MidasNet in its order: per convolution its weight, then its batch norm's
    weight, bias, running_mean, running_var and num_batches_tracked (624 keys for ResNeXt-101 32x8d)."""
    keys = []
    for c in resnext_conv_table(blocks, groups, width_per_group):
        keys.append(prefix + c.key + ".weight")
        keys.extend(prefix + c.norm_key + "." + v for v in RESNEXT_NORM_VECTORS + ("num_batches_tracked",))
    return keys


def resnext_split(K, HWo, kernel_size=1):
    """The split count S of a dense convolution of csrc/cvd_resnext.h (rxSplit there) with K = in_channels kernel_size^2 whose OUTPUT
    has HWo pixels per image: as many slices of K as bring the 64-pixel tiles of one image to 64 workgroups per channel tile, each
    slice whole chains (8 chunks of 32 k for 1 x 1, 3 chunks of 98 for 7 x 7), at most 32.  A function of K and HWo alone."""
    chunk_k, fold = (32, 8) if int(kernel_size) == 1 else (98, 3)
    chunks = (int(K) + chunk_k - 1) // chunk_k
    chains = (chunks + fold - 1) // fold
    tiles = (int(HWo) + 63) // 64
    want = max(1, min(64 // tiles, RESNEXT_MAX_SPLIT, chains))
    per = (chains + want - 1) // want
    return (chains + per - 1) // per


def _resnext_norm(who, norm_shapes, eps, N):
    if norm_shapes is None:
        return
    got = [tuple(int(v) for v in s) for s in norm_shapes]
    if len(got) != 4 or any(g != (N,) for g in got):
        raise ValueError(f"{who}: the norm must be the four vectors {RESNEXT_NORM_VECTORS} of shape ({N},) (got {got})")
    if not eps > 0:
        raise ValueError(f"{who}: eps must be > 0 (got {eps})")


def _resnext_stride(who, stride):
    stride = stride[0] if isinstance(stride, (tuple, list)) and len(set(stride)) == 1 else stride
    if stride not in (1, 2):
        raise ValueError(f"{who}: stride must be 1 or 2 (got {stride})")
    return int(stride)


def resnext_check_grouped_conv(x_shape, weight_shape, stride=1, norm_shapes=None, eps=RESNEXT_EPS):
    """(B, H, W, groups, Cg, Ho, Wo) of the grouped 3 x 3 convolution: x [B, G Cg, H, W], weight [G Cg, Cg, 3, 3] with Cg in
    RESNEXT_GROUP_WIDTHS, stride 1 or 2, padding 1, the norm's four [G Cg] vectors or None.  ValueError (before any device work) for
    anything else."""
    who = "ResNeXt grouped conv"
    B, Cn, H, W = _midas_shape4(who, "x", x_shape)
    ws = tuple(int(v) for v in weight_shape)
    if len(ws) != 4 or ws[2:] != (3, 3):
        raise ValueError(f"{who}: the filter must be 3 x 3 (weight {ws})")
    if ws[0] != Cn:
        raise ValueError(f"{who}: x has {Cn} channels, the weight {ws} writes {ws[0]} (in and out channels are equal)")
    cg = ws[1]
    if cg < 1 or Cn % cg:
        raise ValueError(f"{who}: {Cn} channels are no whole groups of the weight's {cg} (weight {ws})")
    if cg not in RESNEXT_GROUP_WIDTHS:
        raise ValueError(f"{who}: channels per group must be one of {RESNEXT_GROUP_WIDTHS} (got {cg})")
    stride = _resnext_stride(who, stride)
    _resnext_norm(who, norm_shapes, eps, Cn)
    return B, H, W, Cn // cg, cg, (H - 1) // stride + 1, (W - 1) // stride + 1


def resnext_check_conv(x_shape, weight_shape, stride=1, norm_shapes=None, eps=RESNEXT_EPS, residual_shape=None, split=0):
    """(B, H, W, Cin, N, k, Ho, Wo) of one dense convolution of csrc/cvd_resnext.h: x [B, Cin, H, W], weight [N, Cin, k, k] with
    (k, stride) in RESNEXT_DENSE_KERNELS, padding k // 2, no bias, the norm's four [N] vectors or None, a residual of the output's
    shape or None, split 0 (the rule) or 1 .. the chunks of K.  ValueError (before any device work) for anything else."""
    who = "ResNeXt conv"
    B, Cn, H, W = _midas_shape4(who, "x", x_shape)
    ws = tuple(int(v) for v in weight_shape)
    stride = _resnext_stride(who, stride)
    if len(ws) != 4 or ws[2] != ws[3] or (ws[2], stride) not in RESNEXT_DENSE_KERNELS:
        raise ValueError(f"{who}: (kernel_size, stride) must be one of {RESNEXT_DENSE_KERNELS} (weight {ws}, stride {stride})")
    if ws[0] < 1:
        raise ValueError(f"{who}: no output channels (weight {ws})")
    if ws[1] != Cn:
        raise ValueError(f"{who}: x has {Cn} channels, the weight {ws} takes {ws[1]}")
    N, k = ws[0], ws[2]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    _resnext_norm(who, norm_shapes, eps, N)
    if residual_shape is not None and tuple(int(v) for v in residual_shape) != (B, N, Ho, Wo):
        raise ValueError(f"{who}: the residual must be {(B, N, Ho, Wo)} (got {tuple(residual_shape)})")
    cc = 32 if k == 1 else 2
    chunks = (Cn + cc - 1) // cc
    if int(split) != split or not 0 <= split <= chunks:
        raise ValueError(f"{who}: split must be 0 (the rule) or 1 .. {chunks}, the chunks of K (got {split})")
    return B, H, W, Cn, N, k, Ho, Wo


def resnext_check_maxpool(x_shape):
    """(B, C, H, W, Ho, Wo) of nn.MaxPool2d(3, 2, 1); ValueError for anything but a non-empty (B, C, H, W)."""
    B, Cn, H, W = _midas_shape4("ResNeXt maxpool", "x", x_shape)
    return B, Cn, H, W, (H - 1) // 2 + 1, (W - 1) // 2 + 1


def resnext_check_backbone(image_shape, blocks, groups, width_per_group, weight_shapes, norm_shapes, eps=RESNEXT_EPS):
    """(B, H, W, table, out_shapes) of the whole backbone: images [B, 3, H, W] with H and W multiples of 32, one weight and four norm
    vectors per convolution of resnext_conv_table(blocks, groups, width_per_group); out_shapes = the four stages' outputs.
    ValueError for anything else."""
    who = "MiDaS backbone"
    table = resnext_conv_table(blocks, groups, width_per_group)
    B, Cn, H, W = _midas_shape4(who, "images", image_shape)
    if Cn != 3:
        raise ValueError(f"{who}: images must have 3 channels (got {Cn})")
    if H % 32 or W % 32:
        raise ValueError(f"{who}: height and width must be multiples of 32 (got {H} x {W})")
    for k in range(4):
        per = (64 << k) * int(width_per_group) // 64
        if per not in RESNEXT_GROUP_WIDTHS:
            raise ValueError(f"{who}: layer{k + 1} has {per} channels per group; {RESNEXT_GROUP_WIDTHS} are built "
                             f"(width_per_group {width_per_group})")
    if not eps > 0:
        raise ValueError(f"{who}: eps must be > 0 (got {eps})")
    if len(weight_shapes) != len(table) or len(norm_shapes) != len(table):
        raise ValueError(f"{who}: {len(table)} weights and norms are expected (got {len(weight_shapes)}, {len(norm_shapes)})")
    for c, w, four in zip(table, weight_shapes, norm_shapes):
        if tuple(int(v) for v in w) != c.weight_shape:
            raise ValueError(f"{who}: {c.name}.weight must be {c.weight_shape} (got {tuple(w)})")
        _resnext_norm(f"{who}: {c.norm}", four, eps, c.out_channels)
    return B, H, W, table, [(B, 256 << k, H >> (k + 2), W >> (k + 2)) for k in range(4)]


# ---- training of the backbone (csrc/cvd_resnext_grad.h) ----------------------------------------------------------
RESNEXT_NORM_CHUNK = 1024              # elements of a channel a slice of a batch norm reduction holds at least
RESNEXT_NORM_MAX_SPLIT = 64
RESNEXT_WGRAD_CHAIN = 256              # output pixels of one chain of the grouped / stem weight gradient
RESNEXT_WGRAD_MAX_SPLIT = 128
RESNEXT_MOMENTUM = 0.1


def resnext_norm_split(channels, count):
    """The slices per channel of a batch norm reduction of csrc/cvd_resnext_grad.h (rxgNormSplit there) over `count` = B H W elements
    of each of `channels` channels: as many as bring the launch to 1024 workgroups, each whole chunks of 1024 elements, at most 64.
    A function of the two sizes alone."""
    chunks = (int(count) + RESNEXT_NORM_CHUNK - 1) // RESNEXT_NORM_CHUNK
    want = max(1, min(1024 // int(channels), RESNEXT_NORM_MAX_SPLIT, chunks))
    per = (chunks + want - 1) // want
    return (chunks + per - 1) // per


def resnext_wgrad_split(pixels, elements):
    """The slices of the grouped 3 x 3 and the stem's weight gradient (rxgWgradSplit there) over `pixels` = B Ho Wo output pixels for
    `elements` weights: as many slices of whole chains of 256 pixels as bring the launch (a thread per weight, 256 a workgroup) to
    1024 workgroups, at most 128.  A function of the two sizes alone."""
    groups = (int(elements) + 255) // 256
    chains = (int(pixels) + RESNEXT_WGRAD_CHAIN - 1) // RESNEXT_WGRAD_CHAIN
    want = max(1, min(1024 // groups, RESNEXT_WGRAD_MAX_SPLIT, chains))
    per = (chains + want - 1) // want
    return (chains + per - 1) // per


def resnext_check_norm_train(c_shape, vector_shapes, eps=RESNEXT_EPS, momentum=RESNEXT_MOMENTUM, training=True, residual_shape=None):
    """(B, N, H, W) of nn.BatchNorm2d on c [B, N, H, W] with the four [N] vectors RESNEXT_NORM_VECTORS; ValueError (before any device
    work) for anything else, for momentum None (the cumulative average has no kernel) and, in training mode, for one value per
    channel, which torch refuses too."""
    who = "ResNeXt norm"
    B, N, H, W = _midas_shape4(who, "c", c_shape)
    _resnext_norm(who, vector_shapes, eps, N)
    if momentum is None:
        raise ValueError(f"{who}: momentum None (the cumulative moving average) has no kernel")
    if not 0.0 <= float(momentum) <= 1.0:
        raise ValueError(f"{who}: momentum must lie in [0, 1] (got {momentum})")
    if training and B * H * W < 2:
        raise ValueError(f"{who}: training mode needs more than 1 value per channel (got c {tuple(c_shape)})")
    if residual_shape is not None and tuple(int(v) for v in residual_shape) != (B, N, H, W):
        raise ValueError(f"{who}: the residual must be {(B, N, H, W)} (got {tuple(residual_shape)})")
    return B, N, H, W


def resnext_check_norm_grad(gy_shape, c_shape, y_shape, vector_shapes, training=True):
    """(B, N, H, W) of the batch norm's backward: gy, c and y (or None) of one shape, mean, invstd and gamma [N]."""
    who = "ResNeXt norm grad"
    B, N, H, W = _midas_shape4(who, "gy", gy_shape)
    for name, s in (("c", c_shape), ("y", y_shape)):
        if s is not None and tuple(int(v) for v in s) != (B, N, H, W):
            raise ValueError(f"{who}: {name} must be {(B, N, H, W)} (got {tuple(s)})")
    got = [tuple(int(v) for v in s) for s in vector_shapes]
    if len(got) != 3 or any(g != (N,) for g in got):
        raise ValueError(f"{who}: mean, invstd and gamma must have shape ({N},) (got {got})")
    if training and B * H * W < 2:
        raise ValueError(f"{who}: training mode needs more than 1 value per channel (got gy {tuple(gy_shape)})")
    return B, N, H, W


def _resnext_grouped_weight(who, channels, weight_shape):
    ws = tuple(int(v) for v in weight_shape)
    if len(ws) != 4 or ws[2:] != (3, 3):
        raise ValueError(f"{who}: the filter must be 3 x 3 (weight {ws})")
    cg = ws[1]
    if ws[0] != channels or cg < 1 or channels % cg:
        raise ValueError(f"{who}: {channels} channels are no whole groups of the weight {ws}")
    if cg not in RESNEXT_GROUP_WIDTHS:
        raise ValueError(f"{who}: channels per group must be one of {RESNEXT_GROUP_WIDTHS} (got {cg})")
    return channels // cg, cg


def _resnext_out_size(who, gy_shape, B, N, H, W, stride):
    want = (B, N, (H - 1) // stride + 1, (W - 1) // stride + 1)
    if tuple(int(v) for v in gy_shape) != want:
        raise ValueError(f"{who}: gy must be {want} for an input of {H} x {W} at stride {stride} (got {tuple(gy_shape)})")


def _resnext_wgrad_split(who, split):
    if int(split) != split or not 0 <= split <= RESNEXT_WGRAD_MAX_SPLIT:
        raise ValueError(f"{who}: split must be 0 (the rule) or 1 .. {RESNEXT_WGRAD_MAX_SPLIT} (got {split})")


def resnext_check_grouped_conv_grad_input(gy_shape, weight_shape, x_size, stride=1):
    """(B, H, W, groups, Cg) of the grouped convolution's input gradient: x_size = (H, W) of its input, gy [B, G Cg, Ho, Wo]."""
    who = "ResNeXt grouped conv grad input"
    B, N, _, _ = _midas_shape4(who, "gy", gy_shape)
    H, W = (int(v) for v in x_size)
    if H < 1 or W < 1:
        raise ValueError(f"{who}: the input size must be >= 1 (got {H} x {W})")
    G, cg = _resnext_grouped_weight(who, N, weight_shape)
    stride = _resnext_stride(who, stride)
    _resnext_out_size(who, gy_shape, B, N, H, W, stride)
    return B, H, W, G, cg


def resnext_check_grouped_conv_grad_weight(gy_shape, x_shape, channels_per_group, stride=1, split=0):
    """(B, H, W, groups, Cg) of the grouped convolution's weight gradient: gy [B, G Cg, Ho, Wo], x [B, G Cg, H, W]."""
    who = "ResNeXt grouped conv grad weight"
    B, N, H, W = _midas_shape4(who, "x", x_shape)
    G, cg = _resnext_grouped_weight(who, N, (N, int(channels_per_group), 3, 3))
    stride = _resnext_stride(who, stride)
    _resnext_out_size(who, gy_shape, B, N, H, W, stride)
    _resnext_wgrad_split(who, split)
    return B, H, W, G, cg


def resnext_check_conv_grad_input(gy_shape, weight_shape, x_size, stride=1, add_shape=None):
    """(B, H, W, Cin, N) of a 1 x 1 convolution's input gradient at stride 1 or 2 (the stem's is not built)."""
    who = "ResNeXt conv grad input"
    B, N, _, _ = _midas_shape4(who, "gy", gy_shape)
    H, W = (int(v) for v in x_size)
    if H < 1 or W < 1:
        raise ValueError(f"{who}: the input size must be >= 1 (got {H} x {W})")
    ws = tuple(int(v) for v in weight_shape)
    stride = _resnext_stride(who, stride)
    if len(ws) != 4 or ws[2:] != (1, 1):
        raise ValueError(f"{who}: kernel_size must be 1: the stem's input gradient is not built (weight {ws})")
    if ws[0] != N or ws[1] < 1:
        raise ValueError(f"{who}: gy has {N} channels, the weight is {ws}")
    _resnext_out_size(who, gy_shape, B, N, H, W, stride)
    if add_shape is not None and tuple(int(v) for v in add_shape) != (B, ws[1], H, W):
        raise ValueError(f"{who}: the addend must be {(B, ws[1], H, W)} (got {tuple(add_shape)})")
    return B, H, W, ws[1], N


def resnext_check_conv_grad_weight(gy_shape, x_shape, kernel_size, stride=1, split=0):
    """(B, H, W, Cin, N, k) of a dense convolution's weight gradient, (k, stride) in RESNEXT_DENSE_KERNELS."""
    who = "ResNeXt conv grad weight"
    B, Cin, H, W = _midas_shape4(who, "x", x_shape)
    stride = _resnext_stride(who, stride)
    if (kernel_size, stride) not in RESNEXT_DENSE_KERNELS:
        raise ValueError(f"{who}: (kernel_size, stride) must be one of {RESNEXT_DENSE_KERNELS} (got {(kernel_size, stride)})")
    gs = tuple(int(v) for v in gy_shape)
    if len(gs) != 4 or gs[1] < 1:
        raise ValueError(f"{who}: gy must be (B, N, Ho, Wo) (got {gs})")
    _resnext_out_size(who, gy_shape, B, gs[1], H, W, stride)
    _resnext_wgrad_split(who, split)
    return B, H, W, Cin, gs[1], int(kernel_size)


def resnext_check_maxpool_grad(x_shape, gy_shape):
    """(B, C, H, W) of the pool's backward: x its input, gy [B, C, Ho, Wo]."""
    who = "ResNeXt maxpool grad"
    B, Cn, H, W = _midas_shape4(who, "x", x_shape)
    _resnext_out_size(who, gy_shape, B, Cn, H, W, 2)
    return B, Cn, H, W


def resnext_block_saved_shapes(batch, height, width, in_channels, mid_channels, out_channels, stride=1, downsample=False):
    """The shapes of the table cvd_resnext_block_train_device fills, for a Bottleneck on x [batch, in_channels, height, width]: per
    convolution (conv1, conv2, conv3 and, with a downsample branch, downsample.0) its raw output c, the saved mean and invstd, and
    the post-activation tensor -- conv3's is the block's output, downsample.0's the identity."""
    B, H, W = int(batch), int(height), int(width)
    stride = _resnext_stride("ResNeXt block", stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    per = [(mid_channels, H, W), (mid_channels, Ho, Wo), (out_channels, Ho, Wo)] + ([(out_channels, Ho, Wo)] if downsample else [])
    out = []
    for n, h, w in per:
        out += [(B, int(n), h, w), (int(n),), (int(n),), (B, int(n), h, w)]
    return out


def resnext_check_block(x_shape, weight_shapes, norm_shapes, stride=1, eps=RESNEXT_EPS, momentum=RESNEXT_MOMENTUM, training=True):
    """(B, H, W, Cin, width, out, groups, stride, downsample, training flags) of one Bottleneck: weights conv1 [width, Cin, 1, 1],
    conv2 [width, Cg, 3, 3], conv3 [out, width, 1, 1] and optionally downsample.0 [out, Cin, 1, 1]; four [N] norm vectors each."""
    who = "ResNeXt block"
    B, Cin, H, W = _midas_shape4(who, "x", x_shape)
    ws = [tuple(int(v) for v in s) for s in weight_shapes]
    if len(ws) not in (3, 4) or len(norm_shapes) != len(ws):
        raise ValueError(f"{who}: three or four weights and as many norms are expected (got {len(ws)}, {len(norm_shapes)})")
    stride = _resnext_stride(who, stride)
    width, out = ws[0][0], ws[2][0]
    if ws[0] != (width, Cin, 1, 1) or ws[2] != (out, width, 1, 1):
        raise ValueError(f"{who}: conv1 / conv3 must be {(width, Cin, 1, 1)} / {(out, width, 1, 1)} (got {ws[0]}, {ws[2]})")
    G, _cg = _resnext_grouped_weight(who, width, ws[1])
    down = len(ws) == 4
    if down and ws[3] != (out, Cin, 1, 1):
        raise ValueError(f"{who}: downsample.0 must be {(out, Cin, 1, 1)} (got {ws[3]})")
    if not down and (stride != 1 or Cin != out):
        raise ValueError(f"{who}: without a downsample branch stride must be 1 and in == out channels (got {stride}, {Cin}, {out})")
    flags = [bool(training)] * len(ws) if isinstance(training, (bool, int)) else [bool(t) for t in training]
    if len(flags) != len(ws):
        raise ValueError(f"{who}: one training flag per norm is expected (got {len(flags)})")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    for i, (n, hw) in enumerate(zip((width, width, out, out), ((H, W), (Ho, Wo), (Ho, Wo), (Ho, Wo)))):
        if i < len(ws):
            resnext_check_norm_train((B, n) + hw, norm_shapes[i], eps, momentum, flags[i])
    return B, H, W, Cin, width, out, G, stride, down, flags


def resnext_saved_bytes(height, width, batch=1, blocks=RESNEXT101_32X8D[0], groups=RESNEXT101_32X8D[1],
                        width_per_group=RESNEXT101_32X8D[2]):
    """Bytes the training forward of the whole backbone keeps for its backward at `batch` images of height x width: the stem's c and
    post-activation and its pooled output, then every block's table (resnext_block_saved_shapes); a block's input is the previous
    block's output and is counted once."""
    import math
    H, W = (int(height) - 1) // 2 + 1, (int(width) - 1) // 2 + 1
    floats = 2 * batch * 64 * H * W + 2 * 64
    H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    floats += batch * 64 * H * W
    cin = 64
    for k, count in enumerate(blocks):
        planes = 64 << k
        mid, out = planes * int(width_per_group) // 64 * int(groups), 4 * planes
        for i in range(count):
            stride = 2 if (i == 0 and k > 0) else 1
            floats += sum(math.prod(s) for s in resnext_block_saved_shapes(batch, H, W, cin, mid, out, stride, i == 0))
            H, W, cin = (H - 1) // stride + 1, (W - 1) // stride + 1, out
    return 4 * floats


class _DeviceArrays:
    """Raw device buffers of the numpy mirror of a `*_device` entry point (null stream, blocking copies); freed on exit."""

    def __init__(self):
        self._hip = _hip_runtime()
        self._bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self._bufs:
            self._hip.hipFree(p)
        self._bufs = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        if self._hip.hipMalloc(C.byref(p), max(int(nbytes), 1)) != 0:
            raise RuntimeError("hipMalloc failed")
        self._bufs.append(p)
        return p

    def upload(self, a):
        p = self.alloc(a.nbytes)
        if a.nbytes and self._hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) != 0:
            raise RuntimeError("hipMemcpy failed")
        return p

    def download(self, p, a):
        if a.nbytes and self._hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, a.nbytes, 2) != 0:
            raise RuntimeError("hipMemcpy failed")
        return a


def adam_record(step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """The scalars of step number `step` (1, 2, ...) of torch.optim.Adam, in double as torch/optim/adam.py forms them."""
    beta1, beta2 = betas
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return ParamRecord(beta1=beta1, beta2=beta2, eps=eps, grad_decay=weight_decay, param_decay=0.0, step=lr / bias_correction1,
                       denom_scale=bias_correction2 ** 0.5, rule=PARAM_RULES["adam"])


def radam_record(step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, degenerated_to_sgd=True):
    """The scalars of step number `step` of the reference's RAdam, in double as optimizer/radam.py:70-95 forms them: the rule is
    picked by N_sma (rectified from 5 on), the rectification is folded into step_size."""
    import math
    beta1, beta2 = betas
    beta2_t = beta2 ** step
    N_sma_max = 2 / (1 - beta2) - 1
    N_sma = N_sma_max - 2 * step * beta2_t / (1 - beta2_t)
    if N_sma >= 5:
        rule = "radam"
        step_size = math.sqrt((1 - beta2_t) * (N_sma - 4) / (N_sma_max - 4) * (N_sma - 2) / N_sma * N_sma_max / (N_sma_max - 2)) / (1 - beta1 ** step)
    elif degenerated_to_sgd:
        rule = "radam_sgd"
        step_size = 1.0 / (1 - beta1 ** step)
    else:
        rule, step_size = "moments", 0.0
    decay = weight_decay * lr if rule != "moments" and weight_decay != 0 else 0.0
    return ParamRecord(beta1=beta1, beta2=beta2, eps=eps, grad_decay=0.0, param_decay=decay, step=step_size * lr, denom_scale=1.0,
                       rule=PARAM_RULES[rule])


def __getattr__(name):
    if name == "PARAM_CHUNK":   # elements per chunk of the multi-tensor tables: CVD_PARAM_CHUNK of the loaded library
        lib = load_library()
        lib.cvd_param_chunk.restype = C.c_int64
        return int(lib.cvd_param_chunk())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def load_library(variant=None):
    """dlopen the in-tree libcvd_hip.so. Raises ImportError (never falls back) when it is not built.  Nothing is read from the
    environment.  `variant` (development tools only, before anything else loaded the library): a profile build
    lib/libcvd_hip_<variant>.so made by robust_cvd_amd.build.build_variant; the chosen path is reported on stderr."""
    global _lib, _variant
    if _lib is not None and variant:
        raise RuntimeError("load_library(variant=...) must be the first load of the library in the process")
    if _lib is None:
        path = _build.LIB
        if variant:
            path = os.path.join(os.path.dirname(path), f"libcvd_hip_{variant}.so")
            sys.stderr.write(f"[robust_cvd_amd] loading the development variant {path}\n")
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). robust_cvd_amd has no CPU fallback.")
        lib = C.CDLL(path)
        lib.cvd_create.restype = C.c_void_p
        lib.cvd_create.argtypes = [C.c_int32]
        lib.cvd_last_error.restype = C.c_char_p
        lib.cvd_last_error.argtypes = [C.c_void_p]
        lib.cvd_num_active_constraints.restype = C.c_int64
        lib.cvd_abi_revision.restype = C.c_int32
        if lib.cvd_abi_revision() != ABI_REVISION:
            raise ImportError(f"{path} was built with ABI revision {lib.cvd_abi_revision()}, this binding is written against "
                              f"{ABI_REVISION} (include/cvd_hip.h: CVD_ABI_REVISION): rebuild the library")
        _lib = lib
        _variant = variant
    return _lib


def loaded_variant():
    """None for the product library, else the development variant this process loaded (`det`: the bit-reproducible build)."""
    return _variant


EXPORTED_SYMBOLS = [
    "cvd_create", "cvd_destroy", "cvd_last_error", "cvd_abi_sizes", "cvd_opt_params_default",
    "cvd_solver_options_default", "cvd_set_solver_options", "cvd_debug_options_default", "cvd_set_debug_options", "cvd_set_generic_kernels", "cvd_comm_unique_id", "cvd_comm_init", "cvd_comm_init_local_group", "cvd_comm_init_phantom", "cvd_set_pair_graph", "cvd_set_video", "cvd_set_depth", "cvd_set_depth_all",
    "cvd_set_pair_constraints", "cvd_set_pair_flows", "cvd_dense_mode_supported", "cvd_set_triplet_constraints", "cvd_set_poses", "cvd_get_poses",
    "cvd_reset_poses", "cvd_reset_depth_xforms", "cvd_reset_spatial_xforms", "cvd_grid_xform_split",
    "cvd_get_xform_desc", "cvd_num_xform_params", "cvd_get_xform_params", "cvd_set_xform_params",
    "cvd_get_pose_params", "cvd_set_pose_params", "cvd_block_size", "cvd_normalize_depth", "cvd_pose_optimization",
    "cvd_pose_optimization_step", "cvd_evaluate", "cvd_sample_pair_constraints", "cvd_get_sampled_constraints", "cvd_sample_triplet_constraints", "cvd_get_sampled_triplet_constraints", "cvd_set_dynamic_masks", "cvd_corner_min_eigenval", "cvd_dynamic_distance", "cvd_apply_depth_xforms", "cvd_depth_param_maps", "cvd_spatial_warp_maps", "cvd_flow_guided_filter", "cvd_bilateral_filter", "cvd_epipolar_static_flags", "cvd_compute_tracks", "cvd_get_tracks", "cvd_flow_consistency_masks", "cvd_consistency_loss", "cvd_consistency_loss_device", "cvd_scene_flow_loss", "cvd_scene_flow_loss_device", "cvd_spatial_losses", "cvd_spatial_losses_device", "cvd_param_chunk", "cvd_parameter_l1", "cvd_parameter_l1_device", "cvd_param_step", "cvd_param_step_device", "cvd_dataset_create", "cvd_dataset_clear", "cvd_dataset_set_colors", "cvd_dataset_set_flows", "cvd_dataset_set_depth_orig", "cvd_dataset_set_cameras", "cvd_dataset_set_xforms", "cvd_dataset_set_maps", "cvd_dataset_batch", "cvd_dataset_batch_device", "cvd_dataset_bad_indices",
    "cvd_raft_corr_pyramid_device", "cvd_raft_corr_lookup_device", "cvd_raft_upsample_flow_device", "cvd_raft_sepconv_gru_device", "cvd_raft_sepconv_gru_timed", "cvd_raft_conv2d_device", "cvd_raft_update_block_device", "cvd_raft_update_block_timed",
    "cvd_raft_encoder_conv_device", "cvd_raft_instance_norm_device", "cvd_raft_encoder_device", "cvd_raft_encoder_timed",
    "cvd_midas_conv_device", "cvd_midas_upsample2x_device", "cvd_midas_head_device", "cvd_midas_decoder_device", "cvd_midas_decoder_timed",
    "cvd_midas_conv_grad_input_device", "cvd_midas_conv_grad_weight_device", "cvd_midas_upsample2x_grad_device", "cvd_midas_head_grad_device",
    "cvd_midas_decoder_train_device", "cvd_midas_decoder_backward_device", "cvd_midas_decoder_backward_timed",
    "cvd_resnext_grouped_conv_device", "cvd_resnext_conv_device", "cvd_resnext_maxpool_device", "cvd_midas_backbone_device", "cvd_midas_backbone_timed",
    "cvd_resnext_norm_train_device", "cvd_resnext_norm_grad_device", "cvd_resnext_grouped_conv_grad_input_device",
    "cvd_resnext_grouped_conv_grad_weight_device", "cvd_resnext_conv_grad_input_device", "cvd_resnext_conv_grad_weight_device",
    "cvd_resnext_maxpool_grad_device", "cvd_resnext_block_train_device", "cvd_resnext_block_backward_device",
    "cvd_get_summary", "cvd_num_records", "cvd_get_records",
    "cvd_get_kernel_times", "cvd_get_comm_times", "cvd_get_dense_times", "cvd_set_kernel_timing", "cvd_num_active_constraints", "cvd_coarse_debug", "cvd_temporal_debug", "cvd_path_info", "cvd_abi_revision",
    "cvd_block_inverse_debug", "cvd_dense_inverse_debug", "cvd_epipolar_debug", "cvd_flow_masks_debug",
    "cvd_product_launch_debug", "cvd_assembly_launch_debug",
]

KERNEL_CLASSES = ["evaluate_assemble", "matvec_pairs", "matvec_finish", "cg_update", "block_inverse", "cost"]


class Solver(Binding):
    def __init__(self, device=0):
        lib = load_library()
        handle = lib.cvd_create(C.c_int32(device))
        if not handle:
            raise RuntimeError("cvd_create failed: " + (lib.cvd_last_error(None) or b"").decode())
        super().__init__(lib, "cvd_", handle)
        self._options = None
        self._debug = None

    def set_options(self, pcg_relative_tolerance=None, pcg_max_iterations=None, verbose=None,
                    coarse_level=None, robust_loss=None, **variants):
        """Options persist per handle: only the fields given change (robust_loss: 0 Cauchy = reference, 1 Huber).  Names of
        cvd_debug_options (force_iterations, force_sharded_path, pcg_lockstep, stall_fused_tail_once, tail_no_row_staging, tail_closes_scalars, asm_force_stage_depth, asm_force_part_units: test / measurement hooks,
        include/cvd_hip_debug.h) are routed to cvd_set_debug_options."""
        debug = {k: variants.pop(k) for k in list(variants) if k in dict(DebugOptions._fields_) and k != "struct_size"}
        if debug:
            d = self._debug
            if d is None:
                d = DebugOptions()
                self._lib.cvd_debug_options_default(C.byref(d))
                self._debug = d
            for k, v in debug.items():
                setattr(d, k, int(v))
            self._check(self._fn("set_debug_options")(self._h, C.byref(d)))
        o = self._options
        if o is None:
            o = SolverOptions()
            self._lib.cvd_solver_options_default(C.byref(o))
            self._options = o
        if pcg_relative_tolerance is not None:
            o.pcg_relative_tolerance = pcg_relative_tolerance
        if pcg_max_iterations is not None:
            o.pcg_max_iterations = pcg_max_iterations
        if verbose is not None:
            o.verbose = int(verbose)
        if coarse_level is not None:
            o.coarse_level = int(coarse_level)
        if robust_loss is not None:
            o.robust_loss = int(robust_loss)
        for k, v in variants.items():  # dense_matrix_free, block_inverse_variant, coarse_*, temporal_*, ...
            if k not in dict(SolverOptions._fields_):
                raise TypeError(f"unknown solver option {k!r}")
            setattr(o, k, float(v) if k in ("coarse_dense_shift", "temporal_weight") else int(v))
        self._check(self._fn("set_solver_options")(self._h, C.byref(o)))

    def set_robust_loss(self, kind):
        """0: ceres::CauchyLoss(robustness) (the reference, lib/PoseOptimizer.cpp:1220); 1: ceres::HuberLoss(robustness)."""
        self.set_options(robust_loss=kind)

    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        load_library().cvd_comm_unique_id(buf)
        return bytes(buf)

    def comm_init(self, rank, world, unique_id: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self._fn("comm_init")(self._h, C.c_int32(rank), C.c_int32(world), buf))

    def comm_init_local_group(self, rank, world, group_key):
        """Test backend of the exchange layer: `world` handles of this process (one host thread each) form a group."""
        self._check(self._fn("comm_init_local_group")(self._h, C.c_int32(rank), C.c_int32(world), C.c_uint64(group_key)))

    def comm_init_phantom(self, rank, world):
        """Measurement aid (tools/shard_sim.py): rank `rank` of a `world`-rank run whose other ranks do not exist."""
        self._check(self._fn("comm_init_phantom")(self._h, C.c_int32(rank), C.c_int32(world)))

    def set_pair_graph(self, pair_frames):
        """Frame pairs of the whole problem (pair-sharded multi-GPU mode): same array on every rank."""
        import numpy as np
        pf = np.ascontiguousarray(pair_frames, dtype=np.int32).reshape(-1, 2)
        self._check(self._fn("set_pair_graph")(self._h, C.c_int32(pf.shape[0]), pf.ctypes.data_as(C.POINTER(C.c_int32))))

    def set_pair_flows(self, pair_frames, flow, mask):
        """Dense mode (the reference's matchSeparation = 0): flow [P, H, W, 2] f32 pixels and mask [P, H, W] u8 of every
        directed pair instead of a constraint list; the kernels read the images directly."""
        import numpy as np
        pf = np.ascontiguousarray(pair_frames, dtype=np.int32).reshape(-1, 2)
        fl = np.ascontiguousarray(flow, dtype=np.float32)
        mk = np.ascontiguousarray(mask, dtype=np.uint8)
        assert fl.shape == (pf.shape[0], self.height, self.width, 2) and mk.shape == fl.shape[:3], (fl.shape, mk.shape)
        self._check(self._fn("set_pair_flows")(self._h, C.c_int32(pf.shape[0]), pf.ctypes.data_as(C.POINTER(C.c_int32)),
                                               fl.ctypes.data_as(C.POINTER(C.c_float)), mk.ctypes.data_as(C.POINTER(C.c_uint8))))

    def set_generic_kernels(self, enabled=True):
        self._check(self._fn("set_generic_kernels")(self._h, C.c_int32(int(enabled))))

    def set_kernel_timing(self, enabled=True, classes=None, sample_every=1):
        """enabled=True times every kernel class; classes=[names] only those (see KERNEL_CLASSES); sample_every=k attaches
        the hot kernel's start/stop event pair to every k-th launch only (a uniform sample of the launches)."""
        mask = int(bool(enabled))
        if classes is not None:
            mask = 0
            for c in classes:
                mask |= 1 << KERNEL_CLASSES.index(c)
            if mask == 1:
                mask |= 1 << 6  # keep it a mask (bit 0 alone would read as 'all')
        mask |= (max(1, min(256, int(sample_every))) - 1) << 8
        self._check(self._fn("set_kernel_timing")(self._h, C.c_int32(mask)))

    def kernel_times(self):
        ms = (C.c_double * 6)()
        n = (C.c_int64 * 6)()
        self._check(self._fn("get_kernel_times")(self._h, ms, n))
        return {k: {"avg_ms": ms[i], "launches": n[i]} for i, k in enumerate(KERNEL_CLASSES)}

    def dense_times(self):
        """Average ms / launches of the dense mode's two pixel-walking kernels of a Jacobian evaluation (see cvd_get_dense_times)."""
        ms = (C.c_double * 2)()
        n = (C.c_int64 * 2)()
        self._check(self._fn("get_dense_times")(self._h, ms, n))
        return {k: {"avg_ms": ms[i], "launches": n[i]} for i, k in enumerate(("dense_walk", "dense_gg"))}

    def comm_times(self):
        """Average ms / counts of the sharded mode's exchange steps (see cvd_get_comm_times)."""
        ms = (C.c_double * 3)()
        n = (C.c_int64 * 3)()
        self._check(self._fn("get_comm_times")(self._h, ms, n))
        return {k: {"avg_ms": ms[i], "count": n[i]} for i, k in enumerate(("evaluate_exchange", "product_exchange", "coarse_exchange"))}

    def consistency_loss(self, depth, extrinsics, intrinsics, pair_frames, flow_ab, flow_ba, weight_ab, weight_ba, warp=None, *,
                         distance="l1", scale=1.0, alpha=1.0, lambdas=(1.0, 0.0, 100.0), grad=False, timing=False):
        """The static terms of the reference's fine-tuning loss (loss/consistency_loss.py ConsistencyLoss) over a table of frames
        and pairs, and its gradient with respect to the depth maps (include/cvd_hip.h cvd_consistency_loss).
        numpy arrays, all float32 or all float64 -- the dtype of `depth` picks the kernels' precision: depth [F, H, W],
        extrinsics [F, 3, 4], intrinsics [F, 4], pair_frames [P, 2], flow_ab / flow_ba [P, 2, H, W] (pixels, planar),
        weight_ab / weight_ba [P, H, W] (or [P, 1, H, W]), warp [F, 2, H, W] pixel offsets or None.  lambdas = (reprojection,
        disparity, depth ratio).  Returns (total, {"reproj", "disp", "depth ratio"}: [P] float64, only the terms whose lambda
        is > 0), then d total / d depth [F, H, W] when grad, then {"forward", "backward"} kernel ms when timing."""
        import numpy as np
        depth = np.asarray(depth)
        if depth.dtype not in (np.float32, np.float64):
            raise TypeError(f"consistency_loss: depth must be float32 or float64 (got {depth.dtype})")
        dt = depth.dtype
        arr = lambda a: np.ascontiguousarray(a, dtype=dt)
        depth = arr(depth)
        assert depth.ndim == 3, depth.shape
        F, H, W = depth.shape
        pf = np.ascontiguousarray(pair_frames, dtype=np.int32).reshape(-1, 2)
        P = pf.shape[0]
        ext, intr = arr(extrinsics), arr(intrinsics)
        fab, fba = arr(flow_ab), arr(flow_ba)
        wab, wba = arr(weight_ab).reshape(-1, H, W), arr(weight_ba).reshape(-1, H, W)
        wp = None if warp is None else arr(warp)
        assert ext.shape == (F, 3, 4) and intr.shape == (F, 4), (ext.shape, intr.shape)
        assert fab.shape == (P, 2, H, W) and fba.shape == (P, 2, H, W), (fab.shape, fba.shape)
        assert wab.shape == (P, H, W) and wba.shape == (P, H, W), (wab.shape, wba.shape)
        assert wp is None or wp.shape == (F, 2, H, W), wp.shape
        desc = consistency_desc(dt == np.float64, F, P, H, W, distance, scale, alpha, lambdas, wp is not None)
        total = C.c_double(0.0)
        terms = np.zeros((max(P, 1), 3), np.float64)
        g = np.zeros((F, H, W), dt) if grad else None
        ms = (C.c_double * 2)()
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._check(self._fn("consistency_loss")(self._h, C.byref(desc), vp(depth), vp(ext), vp(intr), vp(wp),
                                                 pf.ctypes.data_as(C.POINTER(C.c_int32)), vp(fab), vp(fba), vp(wab), vp(wba),
                                                 C.byref(total), terms.ctypes.data_as(C.POINTER(C.c_double)), vp(g),
                                                 ms if timing else None))
        out = (total.value, {k: terms[:P, i].copy() for i, k in enumerate(CONSISTENCY_TERMS) if lambdas[i] > 0})
        if grad:
            out += (g,)
        if timing:
            out += ({"forward": ms[0], "backward": ms[1]},)
        return out

    def scene_flow_loss(self, depth, extrinsics, intrinsics, pair_frames, flows=None, masks=None, neighbor_frames=None,
                        neighbor_flows=None, neighbor_masks=None, valid=None, warp=None, *, distance_static="l1",
                        distance_smooth="l1", scale=1.0, alpha=1.0, lambdas=(1.0, 1.0, 0.0, 100.0), grad=False, maps=False,
                        timing=False):
        """The reference's SceneFlowLoss (loss/scene_flow_loss.py) over a table of frames and pairs, and its gradient with respect
        to the depth maps (include/cvd_hip.h cvd_scene_flow_loss).  numpy arrays, all float32 or all float64 --
        the dtype of `depth` picks the kernels' precision: depth [F, H, W], extrinsics [F, 3, 4], intrinsics [F, 4], pair_frames
        [P, 2]; flows / masks: 2 arrays [P, 2, H, W] / [P, H, W] (or [P, 1, H, W]) per direction, None when lambdas[0] is 0;
        neighbor_frames [P, 4] = (a-1, a+1, b-1, b+1), neighbor_flows / neighbor_masks: 4 arrays in that order, valid [P, 2], all
        None when the three smooth lambdas are 0; warp [F, 2, H, W] pixel offsets or None.  lambdas = (static, smooth
        reprojection, smooth disparity, smooth depth ratio).  Returns (total, {term: [P] float64} of the terms whose lambda is
        > 0), then d total / d depth [F, H, W] when grad, then the six visualisation maps [6, P, 3, H, W] when maps, then
        {"forward", "backward"} kernel ms when timing."""
        import numpy as np
        depth = np.asarray(depth)
        if depth.dtype not in (np.float32, np.float64):
            raise TypeError(f"scene_flow_loss: depth must be float32 or float64 (got {depth.dtype})")
        dt = depth.dtype
        arr = lambda a: np.ascontiguousarray(a, dtype=dt)
        depth = arr(depth)

        def shaped(name, a, shape):
            if a.shape != shape:
                raise ValueError(f"scene_flow_loss: {name} has shape {a.shape}, expected {shape}")
            return a
        if depth.ndim != 3:
            raise ValueError(f"scene_flow_loss: depth has shape {depth.shape}, expected [F, H, W]")
        F, H, W = depth.shape
        pf = np.ascontiguousarray(pair_frames, dtype=np.int32).reshape(-1, 2)
        P = pf.shape[0]
        ext, intr = shaped("extrinsics", arr(extrinsics), (F, 3, 4)), shaped("intrinsics", arr(intrinsics), (F, 4))
        wp = None if warp is None else shaped("warp", arr(warp), (F, 2, H, W))
        keep = [depth, ext, intr, wp, pf]   # the converted arrays live until the call returns

        def group(name, arrays, n, shape):
            """pointer array of the n arrays of one argument, or None (the library names a missing group an enabled term needs)"""
            if arrays is None:
                return None
            arrays = list(arrays)
            if len(arrays) != n:
                raise ValueError(f"scene_flow_loss: {name} has {len(arrays)} arrays, expected {n}")
            conv = [shaped(f"{name}[{k}]", arr(a).reshape((-1,) + shape[1:]), shape) for k, a in enumerate(arrays)]
            keep.extend(conv)
            return (C.c_void_p * n)(*[a.ctypes.data for a in conv])

        fl, mk = group("flows", flows, 2, (P, 2, H, W)), group("masks", masks, 2, (P, H, W))
        nfl = group("neighbor_flows", neighbor_flows, 4, (P, 2, H, W))
        nmk = group("neighbor_masks", neighbor_masks, 4, (P, H, W))
        nf = None if neighbor_frames is None else shaped(
            "neighbor_frames", np.ascontiguousarray(neighbor_frames, dtype=np.int32).reshape(-1, 4), (P, 4))
        vl = None if valid is None else shaped("valid", arr(valid).reshape(-1, 2), (P, 2))
        desc = scene_flow_desc(dt == np.float64, F, P, H, W, distance_static, distance_smooth, scale, alpha, lambdas,
                               wp is not None)
        total = C.c_double(0.0)
        terms = np.zeros((max(P, 1), 4), np.float64)
        g = np.zeros((F, H, W), dt) if grad else None
        mp = np.zeros((6, max(P, 1), 3, H, W), dt) if maps else None
        ms = (C.c_double * 2)()
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._fn("scene_flow_loss")(self._h, C.byref(desc), vp(depth), vp(ext), vp(intr), vp(wp), ip(pf), fl, mk,
                                                ip(nf), nfl, nmk, vp(vl), C.byref(total),
                                                terms.ctypes.data_as(C.POINTER(C.c_double)), vp(g), vp(mp),
                                                ms if timing else None))
        out = (total.value, {k: terms[:P, i].copy() for i, k in enumerate(SCENE_FLOW_TERMS) if lambdas[i] > 0})
        if grad:
            out += (g,)
        if maps:
            out += (mp[:, :P],)
        if timing:
            out += ({"forward": ms[0], "backward": ms[1]},)
        return out

    def spatial_losses(self, depth, depth_orig=None, image=None, *, frames_per_sample, lambda_disparity_smooth=0.0,
                       sigma_color_grad=1.0, lambda_contrast_loss=0.0, contrast_thresh=1.05, grad=False, timing=False):
        """The reference's DisparitySmoothLoss and ContrastLoss (loss/disparity_smooth_loss.py, loss/contrast_loss.py) over a table
        of frames in one pass, and the gradient with respect to the depth maps (include/cvd_hip.h cvd_spatial_losses, DESIGN.md
        §3.12).  numpy arrays, all float32 or all float64 -- the dtype of `depth` picks the kernels' precision: depth [F, H, W]
        (or [B, N, H, W]), depth_orig likewise (None when lambda_contrast_loss is 0), image [F, 3, H, W] (or [B, N, 3, H, W]; None
        when lambda_disparity_smooth is 0).  Frame f belongs to sample f // frames_per_sample.  Returns (total, smooth [B]
        float64, contrast), then d total / d depth [F, H, W] when grad, then the kernel ms when timing."""
        import numpy as np
        depth = np.asarray(depth)
        if depth.dtype not in (np.float32, np.float64):
            raise TypeError(f"spatial_losses: depth must be float32 or float64 (got {depth.dtype})")
        dt = depth.dtype
        if depth.ndim not in (3, 4):
            raise ValueError(f"spatial_losses: depth has shape {depth.shape}, expected [F, H, W]")
        H, W = depth.shape[-2:]
        depth = np.ascontiguousarray(depth).reshape(-1, H, W)
        F = depth.shape[0]

        def table(name, a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            if a.size != int(np.prod(shape)) or a.shape[-2:] != (H, W):
                raise ValueError(f"spatial_losses: {name} has shape {a.shape}, expected {shape}")
            return a.reshape(shape)
        do = table("depth_orig", depth_orig, (F, H, W))
        im = table("image", image, (F, 3, H, W))
        N = int(frames_per_sample)
        desc = spatial_desc(dt == np.float64, F, N, H, W, lambda_disparity_smooth, sigma_color_grad, lambda_contrast_loss,
                            contrast_thresh)
        total, contrast = C.c_double(0.0), C.c_double(0.0)
        smooth = np.zeros(max(F // max(N, 1), 1), np.float64)
        g = np.zeros((F, H, W), dt) if grad else None
        ms = (C.c_double * 1)()
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._check(self._fn("spatial_losses")(self._h, C.byref(desc), vp(depth), vp(do), vp(im), C.byref(total),
                                               smooth.ctypes.data_as(C.POINTER(C.c_double)), C.byref(contrast), vp(g),
                                               ms if timing else None))
        out = (total.value, smooth[:F // N].copy(), contrast.value)
        if grad:
            out += (g,)
        if timing:
            out += (ms[0],)
        return out

    @staticmethod
    def _param_layout(who, arrays, counts, offsets):
        """The flat arrays of a parameter table, all of one dtype (float32 or float64), with their counts and offsets (default:
        back to back) as int64."""
        import numpy as np
        flat = [np.ascontiguousarray(a).reshape(-1) for a in arrays]
        dt = flat[0].dtype
        if dt not in (np.float32, np.float64):
            raise TypeError(f"{who}: the arrays must be float32 or float64 (got {dt})")
        for a in flat[1:]:
            if a.dtype != dt or a.size != flat[0].size:
                raise ValueError(f"{who}: flat arrays of {a.dtype} x {a.size} and {dt} x {flat[0].size}")
        counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]) if counts.size else np.zeros(0)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if offsets.size != counts.size:
            raise ValueError(f"{who}: {offsets.size} offsets for {counts.size} counts")
        return flat, dt, counts, offsets

    def parameter_l1(self, p, p0, counts, lam, *, offsets=None, grad=None, grad_out=1.0, timing=False):
        """The reference's ParameterLoss (loss/parameter_loss.py) over a list of tensors in one launch, and its subgradient
        (include/cvd_hip.h cvd_parameter_l1).  p, p0: flat numpy arrays, float32 or float64; tensor i is
        counts[i] elements at offsets[i] (default: back to back).  grad: None (value only), True (the gradient lam sign(p - p0)
        grad_out, zero between the tensors) or a flat array the gradient is ADDED to (a copy: the argument stays).  Returns
        total, then the flat gradient when grad, then {"forward", "backward"} kernel ms when timing."""
        import numpy as np
        (p, p0), dt, counts, offsets = self._param_layout("parameter_l1", (p, p0), counts, offsets)
        accumulate = grad is not None and grad is not True
        g = None
        if accumulate:
            g = np.array(grad, dtype=dt).reshape(-1)
            if g.size != p.size:
                raise ValueError(f"parameter_l1: grad has {g.size} elements, the flat arrays {p.size}")
        elif grad:
            g = np.zeros(p.size, dt)
        desc = param_desc(dt == np.float64, counts.size)
        total = C.c_double(0.0)
        ms = (C.c_double * 2)()
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        self._check(self._fn("parameter_l1")(self._h, C.byref(desc), ip(offsets), ip(counts), C.c_int64(p.size), vp(p), vp(p0),
                                             C.c_double(lam), C.byref(total), vp(g), C.c_double(grad_out),
                                             C.c_int32(int(accumulate)), ms if timing else None))
        out = (total.value,)
        if g is not None:
            out += (g,)
        if timing:
            out += ({"forward": ms[0], "backward": ms[1]},)
        return out if len(out) > 1 else out[0]

    def param_step(self, p, g, m, v, counts, records, *, offsets=None, timing=False):
        """One optimizer step of a list of tensors in one launch (include/cvd_hip.h cvd_param_step): flat numpy
        arrays laid out as in parameter_l1, records: one ParamRecord per tensor (adam_record / radam_record), or one for all.
        Returns the new (p, m, v) (copies: the arguments stay), then the kernel ms when timing."""
        import numpy as np
        (p, g, m, v), dt, counts, offsets = self._param_layout("param_step", (p, g, m, v), counts, offsets)
        p, m, v = p.copy(), m.copy(), v.copy()
        if isinstance(records, ParamRecord):
            records = [records] * counts.size
        if len(records) != counts.size:
            raise ValueError(f"param_step: {len(records)} records for {counts.size} tensors")
        rec = (ParamRecord * max(counts.size, 1))(*records)
        desc = param_desc(dt == np.float64, counts.size)
        ms = (C.c_double * 1)()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        self._check(self._fn("param_step")(self._h, C.byref(desc), ip(offsets), ip(counts), C.c_int64(p.size), vp(p), vp(g), vp(m),
                                           vp(v), rec, ms if timing else None))
        return (p, m, v, ms[0]) if timing else (p, m, v)

    # -- fine-tuning batches from a device-resident dataset (include/cvd_hip.h cvd_dataset_*) ---------------
    def dataset_create(self, num_frames, height, width, pair_frames, samples, temporal, has_depth_orig=False,
                       neighbor_rule_frames=0, desc=None):
        """Allocates the store and builds its sample table: pair_frames [Q, 2] directed pairs (slot = position), samples [S, 2].
        desc: a cvd_dataset_desc to pass as it is (tests)."""
        import numpy as np
        pf = np.ascontiguousarray(pair_frames, dtype=np.int32).reshape(-1, 2)
        sm = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1, 2)
        if desc is None:
            desc = dataset_desc(num_frames, height, width, pf.shape[0], sm.shape[0], temporal, has_depth_orig, neighbor_rule_frames)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._fn("dataset_create")(self._h, C.byref(desc), ip(pf), ip(sm)))
        self._dataset = {"F": int(num_frames), "H": int(height), "W": int(width), "Q": pf.shape[0], "S": sm.shape[0],
                         "N": 6 if temporal else 2, "depth_orig": bool(has_depth_orig), "scale_mode": 0, "warp": False}

    def dataset_clear(self):
        self._check(self._fn("dataset_clear")(self._h))
        self._dataset = None

    def _dataset_info(self):
        info = getattr(self, "_dataset", None)
        if info is None:   # (the library names the missing store)
            info = {"F": 0, "H": 1, "W": 1, "Q": 0, "S": 0, "N": 2, "depth_orig": False, "scale_mode": 0, "warp": False}
        return info

    def dataset_set_colors(self, first, hwc3):
        """Colour of frames first, first + 1, ...: float32 [n, H, W, 3], in the channel order the batch returns."""
        import numpy as np
        d = self._dataset_info()
        a = np.ascontiguousarray(hwc3, dtype=np.float32)
        assert a.ndim == 4 and a.shape[1:] == (d["H"], d["W"], 3), a.shape
        self._check(self._fn("dataset_set_colors")(self._h, C.c_int32(first), C.c_int32(a.shape[0]), a.ctypes.data_as(C.c_void_p)))

    def dataset_set_flows(self, first, flow, mask):
        """Flow float32 [n, H, W, 2] and mask uint8 [n, H, W] (file layout) of pair slots first, first + 1, ..."""
        import numpy as np
        d = self._dataset_info()
        fl = np.ascontiguousarray(flow, dtype=np.float32)
        mk = np.ascontiguousarray(mask, dtype=np.uint8)
        assert fl.ndim == 4 and fl.shape[1:] == (d["H"], d["W"], 2) and mk.shape == fl.shape[:3], (fl.shape, mk.shape)
        self._check(self._fn("dataset_set_flows")(self._h, C.c_int32(first), C.c_int32(fl.shape[0]), fl.ctypes.data_as(C.c_void_p),
                                                  mk.ctypes.data_as(C.c_void_p)))

    def dataset_set_depth_orig(self, first, depth):
        """Initial depth (1 / disparity) float32 [n, H, W] of frames first, first + 1, ..."""
        import numpy as np
        d = self._dataset_info()
        a = np.ascontiguousarray(depth, dtype=np.float32)
        assert a.ndim == 3 and a.shape[1:] == (d["H"], d["W"]), a.shape
        self._check(self._fn("dataset_set_depth_orig")(self._h, C.c_int32(first), C.c_int32(a.shape[0]), a.ctypes.data_as(C.c_void_p)))

    def dataset_set_cameras(self, extrinsics, intrinsics):
        import numpy as np
        d = self._dataset_info()
        ext = np.ascontiguousarray(extrinsics, dtype=np.float32)
        intr = np.ascontiguousarray(intrinsics, dtype=np.float32)
        assert ext.shape == (d["F"], 3, 4) and intr.shape == (d["F"], 4), (ext.shape, intr.shape)
        self._check(self._fn("dataset_set_cameras")(self._h, ext.ctypes.data_as(C.c_void_p), intr.ctypes.data_as(C.c_void_p)))

    def dataset_set_xforms(self, depth_desc, depth_params, spatial_desc, spatial_params):
        """The store's scale and warp tables from the transforms' parameters, on the device: depth_params [F, nD], spatial_params
        [F, nS] float64 (None or empty where the transform has none)."""
        import numpy as np
        d = self._dataset_info()
        conv = lambda p: None if p is None or np.size(p) == 0 else np.ascontiguousarray(p, dtype=np.float64).reshape(d["F"], -1)
        dp, sp = conv(depth_params), conv(spatial_params)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._check(self._fn("dataset_set_xforms")(self._h, C.byref(depth_desc), vp(dp), C.byref(spatial_desc), vp(sp)))
        d["scale_mode"] = 2 if int(depth_desc.depth_type) == 3 else 1
        d["warp"] = True

    def dataset_set_maps(self, scales=None, warp=None):
        """The same tables from host arrays: scales float32 [F, H, W] (maps) or F values (anything that reshapes to [F]), warp
        float32 [F, 2, H, W]; None = not set."""
        import numpy as np
        d = self._dataset_info()
        sc = wp = None
        is_map = False
        if scales is not None:
            sc = np.ascontiguousarray(scales, dtype=np.float32)
            is_map = sc.size != d["F"]
            assert sc.size == (d["F"] * d["H"] * d["W"] if is_map else d["F"]), sc.shape
        if warp is not None:
            wp = np.ascontiguousarray(warp, dtype=np.float32)
            assert wp.shape == (d["F"], 2, d["H"], d["W"]), wp.shape
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._check(self._fn("dataset_set_maps")(self._h, vp(sc), C.c_int32(int(is_map)), vp(wp)))
        d["scale_mode"] = 0 if sc is None else (2 if is_map else 1)
        d["warp"] = wp is not None

    def dataset_batch(self, indices, timing=False, device_entry=False, nested=True):
        """One batch as numpy arrays: (images, metadata) with the reference's nesting (nested=False: the flat dict of
        dataset_batch_shapes), plus the kernel ms when timing.  device_entry=True goes through cvd_dataset_batch_device with
        indices and outputs in raw device buffers, on the null stream (tests: that entry point checks no index)."""
        import numpy as np
        d = self._dataset_info()
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        B = idx.size
        shapes = dataset_batch_shapes(max(B, 1), d["N"], d["H"], d["W"], d["scale_mode"], d["warp"], d["depth_orig"])
        flat = {k: np.zeros(shape, dtype) for k, (shape, dtype) in shapes.items()}
        ip = idx.ctypes.data_as(C.POINTER(C.c_int64))
        if not device_entry:
            ms = (C.c_double * 1)()
            out = dataset_batch_out({k: a.ctypes.data for k, a in flat.items()})
            self._check(self._fn("dataset_batch")(self._h, C.c_int32(B), ip, C.byref(out), ms if timing else None))
        else:
            if timing:
                raise ValueError("dataset_batch: the device entry point is not timed")
            hip = _hip_runtime()
            bufs = {}

            def alloc(name, nbytes):
                p = C.c_void_p()
                if hip.hipMalloc(C.byref(p), max(nbytes, 1)) != 0:
                    raise RuntimeError("hipMalloc failed")
                bufs[name] = p
                return p
            try:
                dev_idx = alloc("indices", idx.nbytes)
                if hip.hipMemcpy(dev_idx, idx.ctypes.data_as(C.c_void_p), idx.nbytes, 1) != 0:
                    raise RuntimeError("hipMemcpy failed")
                out = dataset_batch_out({k: alloc(k, a.nbytes).value for k, a in flat.items()})
                self._check(self._fn("dataset_batch_device")(self._h, C.c_int32(B), C.cast(dev_idx, C.POINTER(C.c_int64)), C.byref(out),
                                                             None))
                for k, a in flat.items():   # (a blocking copy on the null stream: behind the launch)
                    if hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), bufs[k], a.nbytes, 2) != 0:
                        raise RuntimeError("hipMemcpy failed")
            finally:
                for p in bufs.values():
                    hip.hipFree(p)
        flat = {k: a[:B] for k, a in flat.items()}
        res = nest_batch(flat) if nested else (flat,)
        return res + (ms[0],) if timing else (res if nested else res[0])

    def dataset_bad_indices(self):
        """Indices the device entry point has clamped since dataset_create (waits for the device)."""
        n = C.c_int64(0)
        self._check(self._fn("dataset_bad_indices")(self._h, C.byref(n)))
        return int(n.value)

    # -- RAFT's correlation pyramid, lookup and convex upsampling (include/cvd_hip.h) on numpy arrays: each goes
    #    through its `*_device` entry point with raw device buffers on the null stream.  Domain errors are ValueErrors, raised
    #    before any device work (api.raft_level_shapes, raft_check_*). ------------------------------------------------------------
    def raft_corr_pyramid(self, raw, dim, levels=4):
        """CorrBlock.__init__ after its matmul: raw [Q, h2, w2] f32 (fmap1^T fmap2) -> the list of `levels` arrays
        [Q, h2 >> l, w2 >> l]; level 0 = raw / sqrt(dim) bit for bit, the others 2 x 2 means."""
        import numpy as np
        raw = np.asarray(raw)
        if raw.dtype != np.float32:
            raise TypeError(f"raft_corr_pyramid: raw must be float32 (got {raw.dtype})")
        if raw.ndim != 3 or min(raw.shape) < 1:
            raise ValueError(f"raft_corr_pyramid: raw must be (Q, h2, w2) (got {raw.shape})")
        raw = np.ascontiguousarray(raw)
        Q, h2, w2 = raw.shape
        shapes = raft_level_shapes(h2, w2, levels)
        dim = raft_check_dim(dim)
        out = [np.zeros((Q, h, w), np.float32) for h, w in shapes]
        with _DeviceArrays() as dev:
            ptrs = [dev.upload(raw)] + [dev.alloc(a.nbytes) for a in out[1:]]
            table = (C.c_void_p * len(ptrs))(*[p.value for p in ptrs])
            self._check(self._fn("raft_corr_pyramid_device")(self._h, C.c_int64(Q), C.c_int32(h2), C.c_int32(w2), C.c_int32(dim),
                                                             C.c_int32(len(shapes)), ptrs[0], table, None))
            for p, a in zip(ptrs, out):
                dev.download(p, a)
        return out

    def raft_corr_lookup(self, levels_list, coords, radius=4):
        """CorrBlock.__call__: levels_list = the pyramid (arrays [Q, h2 >> l, w2 >> l] f32, Q = B h1 w1), coords [B, 2, h1, w1]
        f32 (channel 0 = x) -> [B, L (2 radius + 1)^2, h1, w1] f32."""
        import numpy as np
        lv = [np.asarray(a) for a in levels_list]
        coords = np.asarray(coords)
        if coords.dtype != np.float32 or any(a.dtype != np.float32 for a in lv):
            raise TypeError("raft_corr_lookup: levels and coords must be float32")
        if coords.ndim != 4 or coords.shape[1] != 2 or min(coords.shape) < 1:
            raise ValueError(f"raft_corr_lookup: coords must be (B, 2, h1, w1) (got {coords.shape})")
        if not lv or lv[0].ndim != 3:
            raise ValueError("raft_corr_lookup: levels_list must hold arrays (Q, h, w)")
        radius = raft_check_radius(radius)
        B, _, h1, w1 = coords.shape
        Q, h2, w2 = lv[0].shape
        shapes = raft_level_shapes(h2, w2, len(lv))
        if Q != B * h1 * w1:
            raise ValueError(f"raft_corr_lookup: {Q} correlation maps for {B} x {h1} x {w1} queries")
        for a, (h, w) in zip(lv, shapes):
            if a.shape != (Q, h, w):
                raise ValueError(f"raft_corr_lookup: a level has shape {a.shape}, expected {(Q, h, w)}")
        n = 2 * radius + 1
        out = np.zeros((B, len(lv) * n * n, h1, w1), np.float32)
        with _DeviceArrays() as dev:
            ptrs = [dev.upload(np.ascontiguousarray(a)) for a in lv]
            table = (C.c_void_p * len(ptrs))(*[p.value for p in ptrs])
            dc = dev.upload(np.ascontiguousarray(coords))
            do = dev.alloc(out.nbytes)
            self._check(self._fn("raft_corr_lookup_device")(self._h, C.c_int32(B), C.c_int32(h1), C.c_int32(w1), C.c_int32(h2),
                                                            C.c_int32(w2), C.c_int32(len(lv)), C.c_int32(radius), table, dc, do, None))
            dev.download(do, out)
        return out

    def raft_upsample_flow(self, flow, mask):
        """RAFT.upsample_flow: flow [N, 2, H, W], mask [N, 576, H, W] f32 -> [N, 2, 8 H, 8 W] f32."""
        import numpy as np
        flow, mask = np.asarray(flow), np.asarray(mask)
        if flow.dtype != np.float32 or mask.dtype != np.float32:
            raise TypeError("raft_upsample_flow: flow and mask must be float32")
        N, H, W = raft_check_upsample(flow.shape, mask.shape)
        out = np.zeros((N, 2, 8 * H, 8 * W), np.float32)
        with _DeviceArrays() as dev:
            df, dm = dev.upload(np.ascontiguousarray(flow)), dev.upload(np.ascontiguousarray(mask))
            do = dev.alloc(out.nbytes)
            self._check(self._fn("raft_upsample_flow_device")(self._h, C.c_int32(N), C.c_int32(H), C.c_int32(W), df, dm, do, None))
            dev.download(do, out)
        return out

    def raft_sepconv_gru(self, h, x, weights, biases):
        """SepConvGRU.forward (raft/core/update.py:37-75): h [B, 128, H, W] f32, x [B, 256, H, W] f32 or a tuple
        of up to three arrays whose channel counts are multiples of 32 and sum to 256 (never concatenated), weights / biases = the
        six of convz1, convr1, convq1, convz2, convr2, convq2 in torch's shapes -> the new h [B, 128, H, W] f32."""
        import numpy as np
        segs = [np.asarray(a) for a in (x if isinstance(x, (tuple, list)) else (x,))]
        h = np.asarray(h)
        weights, biases = [np.asarray(a) for a in weights], [np.asarray(a) for a in biases]
        for a in [h] + segs + weights + biases:
            if a.dtype != np.float32:
                raise TypeError(f"raft_sepconv_gru: every array must be float32 (got {a.dtype})")
        B, H, W = raft_check_gru(h.shape, [a.shape for a in segs], [a.shape for a in weights], [a.shape for a in biases])
        out = np.zeros((B, GRU_HIDDEN, H, W), np.float32)
        with _DeviceArrays() as dev:
            dh = dev.upload(np.ascontiguousarray(h))
            ds = [dev.upload(np.ascontiguousarray(a)) for a in segs]
            dw = [dev.upload(np.ascontiguousarray(a)) for a in weights]
            db = [dev.upload(np.ascontiguousarray(a)) for a in biases]
            do = dev.alloc(out.nbytes)
            seg_table = (C.c_void_p * len(ds))(*[p.value for p in ds])
            seg_channels = (C.c_int32 * len(ds))(*[a.shape[1] for a in segs])
            w_table, b_table = (C.c_void_p * 6)(*[p.value for p in dw]), (C.c_void_p * 6)(*[p.value for p in db])
            self._check(self._fn("raft_sepconv_gru_device")(self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), dh, C.c_int32(len(ds)),
                                                            seg_table, seg_channels, w_table, b_table, do, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("raft_sepconv_gru: the device reported an error")
            dev.download(do, out)
        return out

    def raft_conv2d(self, x, weights, biases, relu=False, scale=1.0, out=None, out_first=0):
        """One convolution of the update block (csrc/cvd_raftconv.h): x [B, C, H, W] f32 or a tuple of up to three
        (channel counts in multiples of 32, never concatenated); weights = one array [O, C, k, k] (k = 1, 3, 7; stride 1, padding
        k // 2) or a list of two alike, stacked along O; biases alike; scale * act(conv + bias).  With `out` [B, C_out, H, W] the
        result goes to its channels out_first .. and the other channels keep their values; the array itself is returned (a copy)."""
        import numpy as np
        segs = [np.asarray(a) for a in (x if isinstance(x, (tuple, list)) else (x,))]
        ws = [np.asarray(a) for a in (weights if isinstance(weights, (tuple, list)) else (weights,))]
        bs = [np.asarray(a) for a in (biases if isinstance(biases, (tuple, list)) else (biases,))]
        given = None if out is None else np.asarray(out)
        for a in segs + ws + bs + ([] if given is None else [given]):
            if a.dtype != np.float32:
                raise TypeError(f"raft_conv2d: every array must be float32 (got {a.dtype})")
        B, H, W, N = raft_check_conv2d([a.shape for a in segs], [a.shape for a in ws], [a.shape for a in bs],
                                       None if given is None else (given.shape[1] if given.ndim == 4 else -1), out_first)
        if given is not None and (given.shape[0], given.shape[2], given.shape[3]) != (B, H, W):
            raise ValueError(f"raft_conv2d: out has shape {given.shape}, expected ({B}, C, {H}, {W})")
        res = np.zeros((B, N, H, W), np.float32) if given is None else np.ascontiguousarray(given).copy()
        with _DeviceArrays() as dev:
            ds = [dev.upload(np.ascontiguousarray(a)) for a in segs]
            dw = [dev.upload(np.ascontiguousarray(a)) for a in ws]
            db = [dev.upload(np.ascontiguousarray(a)) for a in bs]
            do = dev.upload(res)
            self._check(self._fn("raft_conv2d_device")(
                self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(len(ds)), (C.c_void_p * len(ds))(*[p.value for p in ds]),
                (C.c_int32 * len(ds))(*[a.shape[1] for a in segs]), C.c_int32(len(dw)), (C.c_void_p * len(dw))(*[p.value for p in dw]),
                (C.c_void_p * len(db))(*[p.value for p in db]), C.c_int32(ws[0].shape[1]), C.c_int32(ws[0].shape[0]),
                C.c_int32(ws[0].shape[2]), C.c_int32(1), C.c_int32(1), C.c_int32(1), C.c_int32(1 if relu else 0), C.c_float(scale),
                do, C.c_int32(res.shape[1]), C.c_int32(out_first), None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("raft_conv2d: the device reported an error")
            dev.download(do, res)
        return res

    def raft_update_block(self, net, inp, corr, flow, weights, biases, compute_mask=True):
        """BasicUpdateBlock.forward (raft/core/update.py:133-156): net, inp [B, 128, H, W], corr
        [B, cor_planes, H, W], flow [B, 2, H, W] f32, weights / biases = the 15 of UPDATE_BLOCK_PARAMETERS in torch's shapes ->
        (net [B, 128, H, W], mask [B, 576, H, W] or None without compute_mask, delta_flow [B, 2, H, W])."""
        import numpy as np
        net, inp, corr, flow = (np.asarray(a) for a in (net, inp, corr, flow))
        weights, biases = [np.asarray(a) for a in weights], [np.asarray(a) for a in biases]
        for a in [net, inp, corr, flow] + weights + biases:
            if a.dtype != np.float32:
                raise TypeError(f"raft_update_block: every array must be float32 (got {a.dtype})")
        B, H, W = raft_check_update_block(net.shape, inp.shape, corr.shape, flow.shape, [a.shape for a in weights],
                                          [a.shape for a in biases])
        net_out = np.zeros((B, GRU_HIDDEN, H, W), np.float32)
        delta = np.zeros((B, 2, H, W), np.float32)
        mask = np.zeros((B, 576, H, W), np.float32) if compute_mask else None
        with _DeviceArrays() as dev:
            dn, di, dc, df = (dev.upload(np.ascontiguousarray(a)) for a in (net, inp, corr, flow))
            dw = [dev.upload(np.ascontiguousarray(a)) for a in weights]
            db = [dev.upload(np.ascontiguousarray(a)) for a in biases]
            do, dd = dev.alloc(net_out.nbytes), dev.alloc(delta.nbytes)
            dm = dev.alloc(mask.nbytes) if compute_mask else None
            self._check(self._fn("raft_update_block_device")(
                self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(corr.shape[1]), C.c_int32(weights[0].shape[1]),
                dn, di, dc, df, (C.c_void_p * 15)(*[p.value for p in dw]), (C.c_void_p * 15)(*[p.value for p in db]), do, dd, dm, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("raft_update_block: the device reported an error")
            dev.download(do, net_out)
            dev.download(dd, delta)
            if compute_mask:
                dev.download(dm, mask)
        return net_out, mask, delta

    def raft_encoder_conv(self, x, weight, bias, stride=1, norm=None, eps=1e-5, relu=False, residual=None):
        """One convolution of RAFT's encoders (csrc/cvd_raftenc.h): x [B, C, H, W] f32, weight [N, C, k, k] (k = 1,
        3, 7), stride 1 or 2, padding k // 2; then + bias, the eval batch norm of `norm` = (weight, bias, running_mean, running_var),
        ReLU, relu(residual + y), each optional -> [B, N, ceil(H / stride), ceil(W / stride)]."""
        import numpy as np
        x, weight, bias = (np.asarray(a) for a in (x, weight, bias))
        norm = None if norm is None else [np.asarray(a) for a in norm]
        residual = None if residual is None else np.asarray(residual)
        for a in [x, weight, bias] + (norm or []) + ([] if residual is None else [residual]):
            if a.dtype != np.float32:
                raise TypeError(f"raft_encoder_conv: every array must be float32 (got {a.dtype})")
        B, H, W, Cin, N, k, Ho, Wo = raft_check_encoder_conv(x.shape, weight.shape, bias.shape, stride,
                                                             None if norm is None else [a.shape for a in norm], eps,
                                                             None if residual is None else residual.shape)
        stride = stride[0] if isinstance(stride, (tuple, list)) else stride
        out = np.zeros((B, N, Ho, Wo), np.float32)
        with _DeviceArrays() as dev:
            dx, dw, db = (dev.upload(np.ascontiguousarray(a)) for a in (x, weight, bias))
            dn = None if norm is None else (C.c_void_p * 4)(*[dev.upload(np.ascontiguousarray(a)).value for a in norm])
            dr = None if residual is None else dev.upload(np.ascontiguousarray(residual))
            do = dev.alloc(out.nbytes)
            self._check(self._fn("raft_encoder_conv_device")(
                self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(Cin), C.c_int32(N), C.c_int32(k), C.c_int32(stride), dx, dw,
                db, dn, C.c_float(eps), C.c_int32(1 if relu else 0), dr, do, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("raft_encoder_conv: the device reported an error")
            dev.download(do, out)
        return out

    def raft_instance_norm(self, x, eps=1e-5, relu=False, residual=None, inplace=False):
        """nn.InstanceNorm2d without affine and running statistics (csrc/cvd_raftenc.h) per (image, channel) plane
        of x [B, C, H, W] f32, then ReLU and relu(residual + y), each optional.  inplace: the device output is the device input
        (the returned array is new either way)."""
        import numpy as np
        x = np.asarray(x)
        residual = None if residual is None else np.asarray(residual)
        for a in [x] + ([] if residual is None else [residual]):
            if a.dtype != np.float32:
                raise TypeError(f"raft_instance_norm: every array must be float32 (got {a.dtype})")
        B, Cn, H, W = raft_check_instance_norm(x.shape, eps, None if residual is None else residual.shape)
        out = np.zeros(x.shape, np.float32)
        with _DeviceArrays() as dev:
            dx = dev.upload(np.ascontiguousarray(x))
            dr = None if residual is None else dev.upload(np.ascontiguousarray(residual))
            do = dx if inplace else dev.alloc(out.nbytes)
            self._check(self._fn("raft_instance_norm_device")(
                self._h, C.c_int32(B), C.c_int32(Cn), C.c_int32(H), C.c_int32(W), dx, C.c_float(eps), C.c_int32(1 if relu else 0), dr,
                do, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("raft_instance_norm: the device reported an error")
            dev.download(do, out)
        return out

    def raft_encoder(self, images, weights, biases, norm="none", norms=None, eps=1e-5, kernel_ms=None):
        """BasicEncoder.forward in eval mode (raft/core/extractor.py:173-197): images [B, 3, H, W] f32 scaled to
        [-1, 1], weights / biases = the 16 of ENCODER_PARAMETERS in torch's shapes, norm in ("none", "instance", "batch"), for
        "batch" norms = 15 x (weight, bias, running_mean, running_var) in ENCODER_NORMS order -> [B, output_dim, ceil(H / 8),
        ceil(W / 8)].  kernel_ms (measurement): a list that receives the 48 per-launch milliseconds of cvd_raft_encoder_timed."""
        import numpy as np
        images = np.asarray(images)
        weights, biases = [np.asarray(a) for a in weights], [np.asarray(a) for a in biases]
        norms = None if norms is None else [[np.asarray(a) for a in four] for four in norms]
        for a in [images] + weights + biases + [a for four in (norms or []) for a in four]:
            if a.dtype != np.float32:
                raise TypeError(f"raft_encoder: every array must be float32 (got {a.dtype})")
        B, H, W, output_dim, mode, (h, w) = raft_check_encoder(images.shape, [a.shape for a in weights], [a.shape for a in biases], norm,
                                                               None if norms is None else [[a.shape for a in four] for four in norms],
                                                               eps)
        out = np.zeros((B, output_dim, h, w), np.float32)
        with _DeviceArrays() as dev:
            di = dev.upload(np.ascontiguousarray(images))
            dw = (C.c_void_p * 16)(*[dev.upload(np.ascontiguousarray(a)).value for a in weights])
            db = (C.c_void_p * 16)(*[dev.upload(np.ascontiguousarray(a)).value for a in biases])
            dn = None
            if norm == "batch":
                dn = (C.c_void_p * 60)(*[dev.upload(np.ascontiguousarray(a)).value for four in norms for a in four])
            do = dev.alloc(out.nbytes)
            args = (self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(output_dim), C.c_int32(mode), C.c_float(eps), di, dw, db,
                    dn, do, None)
            if kernel_ms is None:
                self._check(self._fn("raft_encoder_device")(*args))
            else:
                ms = (C.c_double * 48)()
                self._check(self._fn("raft_encoder_timed")(*args, ms))
                kernel_ms[:] = list(ms)
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("raft_encoder: the device reported an error")
            dev.download(do, out)
        return out

    @staticmethod
    def _midas_f32(who, arrays):
        import numpy as np
        for a in arrays:
            if a is not None and a.dtype != np.float32:
                raise TypeError(f"{who}: every array must be float32 (got {a.dtype})")

    def midas_conv(self, x, weight, bias=None, relu_in=False, relu=False, a=None, relu_a=False, b=None, split=0):
        """One convolution of the MiDaS decoder (csrc/cvd_midas.h): x [B, C, H, W] f32, weight [N, C, k, k] (k = 1,
        3), stride 1, padding k // 2 -> [B, N, H, W]: t = conv(max(x, 0) under relu_in, else x) + bias (or none); max(t, 0) under
        relu; t + (max(a, 0) under relu_a, else a) with an addend a; b + t with a second addend b.  split: 0 = the rule
        (midas_split), else the forced number of slices of K."""
        import numpy as np
        x, weight = np.asarray(x), np.asarray(weight)
        bias, a, b = (None if v is None else np.asarray(v) for v in (bias, a, b))
        self._midas_f32("midas_conv", [x, weight, bias, a, b])
        B, H, W, Cin, N, k = midas_check_conv(x.shape, weight.shape, None if bias is None else bias.shape,
                                              None if a is None else a.shape, None if b is None else b.shape, split)
        out = np.zeros((B, N, H, W), np.float32)
        with _DeviceArrays() as dev:
            dx, dw = dev.upload(np.ascontiguousarray(x)), dev.upload(np.ascontiguousarray(weight))
            db, da, d2 = (None if v is None else dev.upload(np.ascontiguousarray(v)) for v in (bias, a, b))
            do = dev.alloc(out.nbytes)
            self._check(self._fn("midas_conv_device")(
                self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(Cin), C.c_int32(N), C.c_int32(k), dx, dw, db,
                C.c_int32(1 if relu_in else 0), C.c_int32(1 if relu else 0), da, C.c_int32(1 if relu_a else 0), d2, C.c_int32(split),
                do, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("midas_conv: the device reported an error")
            dev.download(do, out)
        return out

    def midas_upsample2x(self, x, align_corners=True):
        """Bilinear x 2 of x [B, C, H, W] f32 as torch.nn.functional.interpolate(scale_factor=2, mode="bilinear", align_corners=...)
        (csrc/cvd_midas.h) -> [B, C, 2 H, 2 W]."""
        import numpy as np
        x = np.asarray(x)
        self._midas_f32("midas_upsample2x", [x])
        B, Cn, H, W = midas_check_upsample2x(x.shape)
        out = np.zeros((B, Cn, 2 * H, 2 * W), np.float32)
        with _DeviceArrays() as dev:
            dx = dev.upload(np.ascontiguousarray(x))
            do = dev.alloc(out.nbytes)
            self._check(self._fn("midas_upsample2x_device")(
                self._h, C.c_int32(B), C.c_int32(Cn), C.c_int32(H), C.c_int32(W), C.c_int32(1 if align_corners else 0), dx, do, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("midas_upsample2x: the device reported an error")
            dev.download(do, out)
        return out

    def midas_head(self, x, weight2, bias2, weight4, bias4, non_negative=True):
        """The output head behind Interpolate in one launch (csrc/cvd_midas.h): x [B, C, H, W] f32, output_conv.2 [32, C, 3, 3] and
        [32], ReLU, output_conv.4 [1, 32, 1, 1] and [1], ReLU under non_negative -> [B, H, W]."""
        import numpy as np
        arrays = [np.asarray(v) for v in (x, weight2, bias2, weight4, bias4)]
        self._midas_f32("midas_head", arrays)
        B, H, W, Cin = midas_check_head(*[v.shape for v in arrays])
        out = np.zeros((B, H, W), np.float32)
        with _DeviceArrays() as dev:
            dx, dw2, db2, dw4, db4 = (dev.upload(np.ascontiguousarray(v)) for v in arrays)
            do = dev.alloc(out.nbytes)
            self._check(self._fn("midas_head_device")(
                self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(Cin), C.c_int32(MIDAS_HEAD_MID), dx, dw2, db2, dw4, db4,
                C.c_int32(1 if non_negative else 0), do, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("midas_head: the device reported an error")
            dev.download(do, out)
        return out

    def midas_conv_grad_input(self, gy, weight, add=None, mask=None, split=0):
        """Input gradient of one convolution of the MiDaS decoder (csrc/cvd_midas_grad.h): gy [B, N, H, W] f32,
        weight [N, C, k, k] -> gx [B, C, H, W] = conv_transpose(gy, weight); + add with an addend; zero where mask <= 0 with a mask.
        split: 0 = the rule (midas_split of K = N k k), else the forced number of slices of K."""
        import numpy as np
        gy, weight = np.asarray(gy), np.asarray(weight)
        add, mask = (None if v is None else np.asarray(v) for v in (add, mask))
        self._midas_f32("midas_conv_grad_input", [gy, weight, add, mask])
        B, H, W, Cin, N, k = midas_check_conv_grad_input(gy.shape, weight.shape, None if add is None else add.shape,
                                                         None if mask is None else mask.shape, split)
        out = np.zeros((B, Cin, H, W), np.float32)
        with _DeviceArrays() as dev:
            dg, dw = dev.upload(np.ascontiguousarray(gy)), dev.upload(np.ascontiguousarray(weight))
            da, dm = (None if v is None else dev.upload(np.ascontiguousarray(v)) for v in (add, mask))
            do = dev.alloc(out.nbytes)
            self._check(self._fn("midas_conv_grad_input_device")(
                self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(Cin), C.c_int32(N), C.c_int32(k), dg, dw, da, dm,
                C.c_int32(split), do, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("midas_conv_grad_input: the device reported an error")
            dev.download(do, out)
        return out

    def midas_conv_grad_weight(self, gy, x, kernel_size, relu_in=False, bias=True, split=0):
        """Weight and bias gradient of one convolution (csrc/cvd_midas_grad.h): gy [B, N, H, W] f32, x [B, C, H, W] the
        convolution's input (rectified first under relu_in) -> (gW [N, C, k, k], gbias [N], or None with bias=False).  split: 0 = the
        rule (midas_wgrad_split), else the forced number of slices of the pixels."""
        import numpy as np
        gy, x = np.asarray(gy), np.asarray(x)
        self._midas_f32("midas_conv_grad_weight", [gy, x])
        B, H, W, Cin, N, k = midas_check_conv_grad_weight(gy.shape, x.shape, kernel_size, split)
        gw = np.zeros((N, Cin, k, k), np.float32)
        gb = np.zeros((N,), np.float32) if bias else None
        with _DeviceArrays() as dev:
            dg, dx = dev.upload(np.ascontiguousarray(gy)), dev.upload(np.ascontiguousarray(x))
            dw = dev.alloc(gw.nbytes)
            db = dev.alloc(gb.nbytes) if bias else None
            self._check(self._fn("midas_conv_grad_weight_device")(
                self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(Cin), C.c_int32(N), C.c_int32(k), dg, dx,
                C.c_int32(1 if relu_in else 0), C.c_int32(split), dw, db, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("midas_conv_grad_weight: the device reported an error")
            dev.download(dw, gw)
            if bias:
                dev.download(db, gb)
        return gw, gb

    def midas_upsample2x_grad(self, gy, align_corners=True):
        """Backward of midas_upsample2x (csrc/cvd_midas_grad.h): gy [B, C, 2 H, 2 W] f32 -> gx [B, C, H, W]."""
        import numpy as np
        gy = np.asarray(gy)
        self._midas_f32("midas_upsample2x_grad", [gy])
        B, Cn, H, W = midas_check_upsample2x_grad(gy.shape)
        out = np.zeros((B, Cn, H, W), np.float32)
        with _DeviceArrays() as dev:
            dg = dev.upload(np.ascontiguousarray(gy))
            do = dev.alloc(out.nbytes)
            self._check(self._fn("midas_upsample2x_grad_device")(
                self._h, C.c_int32(B), C.c_int32(Cn), C.c_int32(H), C.c_int32(W), C.c_int32(1 if align_corners else 0), dg, do, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("midas_upsample2x_grad: the device reported an error")
            dev.download(do, out)
        return out

    def midas_decoder_train(self, maps, weights, biases, non_negative=True):
        """midas_decoder that also returns the activations the backward needs (cvd_midas_decoder_train_device): -> (out [B, H, W],
        saved: the 16 arrays of midas_saved_shapes).  out equals midas_decoder's bit for bit."""
        import numpy as np
        maps, weights, biases = ([np.asarray(a) for a in v] for v in (maps, weights, biases))
        self._midas_f32("midas_decoder_train", maps + weights + biases)
        B, features, channels, heights, widths = midas_check_decoder([v.shape for v in maps], [v.shape for v in weights],
                                                                         [v.shape for v in biases])
        out = np.zeros((B, 4 * heights[0], 4 * widths[0]), np.float32)
        saved = [np.zeros(s, np.float32) for s in midas_saved_shapes(B, features, heights, widths)]
        with _DeviceArrays() as dev:
            up = lambda arrays: [dev.upload(np.ascontiguousarray(a)).value for a in arrays]
            dm, dw, db = (C.c_void_p * 4)(*up(maps)), (C.c_void_p * 21)(*up(weights)), (C.c_void_p * 17)(*up(biases))
            dsv = [dev.alloc(a.nbytes) for a in saved]
            do = dev.alloc(out.nbytes)
            self._check(self._fn("midas_decoder_train_device")(
                self._h, C.c_int32(B), C.c_int32(features), (C.c_int32 * 4)(*channels), (C.c_int32 * 4)(*heights), (C.c_int32 * 4)(*widths),
                dm, dw, db, C.c_int32(1 if non_negative else 0), (C.c_void_p * MIDAS_SAVED)(*[p.value for p in dsv]), do, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("midas_decoder_train: the device reported an error")
            dev.download(do, out)
            for p, a in zip(dsv, saved):
                dev.download(p, a)
        return out, saved

    def midas_decoder_backward(self, gy, maps, saved, weights, biases, non_negative=True, map_gradients=True, kernel_ms=None):
        """The decoder's backward in one library call (cvd_midas_decoder_backward_device): gy [B, H, W] f32, the feature maps, the
        saved table of midas_decoder_train and the parameters -> (weight gradients (21), bias gradients (17), map gradients (4) or
        None with map_gradients=False).  kernel_ms: a list that receives cvd_midas_decoder_backward_timed's milliseconds."""
        import numpy as np
        gy = np.asarray(gy)
        maps, saved, weights, biases = ([np.asarray(a) for a in v] for v in (maps, saved, weights, biases))
        self._midas_f32("midas_decoder_backward", [gy] + maps + saved + weights + biases)
        B, features, channels, heights, widths = midas_check_decoder([v.shape for v in maps], [v.shape for v in weights],
                                                                         [v.shape for v in biases])
        if tuple(gy.shape) != (B, 4 * heights[0], 4 * widths[0]):
            raise ValueError(f"MiDaS decoder backward: gy must be {(B, 4 * heights[0], 4 * widths[0])} (got {tuple(gy.shape)})")
        want = midas_saved_shapes(B, features, heights, widths)
        if [tuple(a.shape) for a in saved] != want:
            raise ValueError(f"MiDaS decoder backward: the saved table must have the shapes {want}")
        gw, gb = [np.zeros(a.shape, np.float32) for a in weights], [np.zeros(a.shape, np.float32) for a in biases]
        gm = [np.zeros(a.shape, np.float32) for a in maps] if map_gradients else None
        with _DeviceArrays() as dev:
            up = lambda arrays: [dev.upload(np.ascontiguousarray(a)).value for a in arrays]
            new = lambda arrays: [dev.alloc(a.nbytes) for a in arrays]
            dg = dev.upload(np.ascontiguousarray(gy))
            dm, dsv = (C.c_void_p * 4)(*up(maps)), (C.c_void_p * MIDAS_SAVED)(*up(saved))
            dw, db = (C.c_void_p * 21)(*up(weights)), (C.c_void_p * 17)(*up(biases))
            pgw, pgb, pgm = new(gw), new(gb), (new(gm) if map_gradients else None)
            args = (self._h, C.c_int32(B), C.c_int32(features), (C.c_int32 * 4)(*channels), (C.c_int32 * 4)(*heights),
                    (C.c_int32 * 4)(*widths), dg, dm, dsv, dw, db, C.c_int32(1 if non_negative else 0),
                    (C.c_void_p * 21)(*[p.value for p in pgw]), (C.c_void_p * 17)(*[p.value for p in pgb]),
                    (C.c_void_p * 4)(*[p.value for p in pgm]) if map_gradients else None, None)
            if kernel_ms is None:
                self._check(self._fn("midas_decoder_backward_device")(*args))
            else:
                ms = (C.c_double * MIDAS_BACKWARD_SLOTS)()
                self._check(self._fn("midas_decoder_backward_timed")(*args, ms))
                kernel_ms[:] = list(ms)
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("midas_decoder_backward: the device reported an error")
            for ptrs, arrays in ((pgw, gw), (pgb, gb)) + (((pgm, gm),) if map_gradients else ()):
                for p, a in zip(ptrs, arrays):
                    dev.download(p, a)
        return gw, gb, gm

    def midas_head_grad(self, gy, x, weight2, bias2, weight4, bias4, non_negative=True):
        """Backward of midas_head (csrc/cvd_midas_grad.h): gy [B, H, W] f32 and the head's inputs -> (gx, gW2, gb2, gW4, gb4) in the
        shapes of x and the four parameters."""
        import numpy as np
        arrays = [np.asarray(v) for v in (x, weight2, bias2, weight4, bias4)]
        gy = np.asarray(gy)
        self._midas_f32("midas_head_grad", arrays + [gy])
        B, H, W, Cin = midas_check_head(*[v.shape for v in arrays])
        if tuple(gy.shape) != (B, H, W):
            raise ValueError(f"MiDaS head grad: gy must be {(B, H, W)} (got {tuple(gy.shape)})")
        outs = [np.zeros(v.shape, np.float32) for v in arrays]
        with _DeviceArrays() as dev:
            dg = dev.upload(np.ascontiguousarray(gy))
            dx, dw2, db2, dw4, db4 = (dev.upload(np.ascontiguousarray(v)) for v in arrays)
            douts = [dev.alloc(o.nbytes) for o in outs]
            self._check(self._fn("midas_head_grad_device")(
                self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(Cin), C.c_int32(MIDAS_HEAD_MID), dg, dx, dw2, db2, dw4, db4,
                C.c_int32(1 if non_negative else 0), *douts, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("midas_head_grad: the device reported an error")
            for d, o in zip(douts, outs):
                dev.download(d, o)
        return tuple(outs)

    def midas_decoder(self, maps, weights, biases, non_negative=True, kernel_ms=None):
        """MidasNet.forward behind the backbone (monodepth/midas_v2/midas_net.py:62-74): maps = the four feature
        maps [B, C_k, H_k, W_k] f32 (layer1 first, each half the one before), weights / biases = the 21 / 17 of MIDAS_PARAMETERS in
        torch's shapes -> [B, 4 H_1, 4 W_1].  kernel_ms (measurement): a list that receives the 44 per-launch milliseconds of
        cvd_midas_decoder_timed."""
        import numpy as np
        maps = [np.asarray(v) for v in maps]
        weights, biases = [np.asarray(v) for v in weights], [np.asarray(v) for v in biases]
        self._midas_f32("midas_decoder", maps + weights + biases)
        B, features, channels, heights, widths = midas_check_decoder([v.shape for v in maps], [v.shape for v in weights],
                                                                     [v.shape for v in biases])
        out = np.zeros((B, 4 * heights[0], 4 * widths[0]), np.float32)
        with _DeviceArrays() as dev:
            dm = (C.c_void_p * 4)(*[dev.upload(np.ascontiguousarray(v)).value for v in maps])
            dw = (C.c_void_p * 21)(*[dev.upload(np.ascontiguousarray(v)).value for v in weights])
            db = (C.c_void_p * 17)(*[dev.upload(np.ascontiguousarray(v)).value for v in biases])
            do = dev.alloc(out.nbytes)
            args = (self._h, C.c_int32(B), C.c_int32(features), (C.c_int32 * 4)(*channels), (C.c_int32 * 4)(*heights),
                    (C.c_int32 * 4)(*widths), dm, dw, db, C.c_int32(1 if non_negative else 0), do, None)
            if kernel_ms is None:
                self._check(self._fn("midas_decoder_device")(*args))
            else:
                ms = (C.c_double * MIDAS_TIMED_SLOTS)()
                self._check(self._fn("midas_decoder_timed")(*args, ms))
                kernel_ms[:] = list(ms)
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("midas_decoder: the device reported an error")
            dev.download(do, out)
        return out

    @staticmethod
    def _resnext_norm(dev, norm):
        import numpy as np
        return None if norm is None else (C.c_void_p * 4)(*[dev.upload(np.ascontiguousarray(a)).value for a in norm])

    def resnext_grouped_conv(self, x, weight, stride=1, norm=None, eps=RESNEXT_EPS, relu=False):
        """nn.Conv2d(G Cg, G Cg, 3, stride, padding=1, groups=G, bias=False) (csrc/cvd_resnext.h): x [B, G Cg, H, W]
        f32, weight [G Cg, Cg, 3, 3], Cg in RESNEXT_GROUP_WIDTHS -> [B, G Cg, Ho, Wo]; norm = (weight, bias, running_mean,
        running_var) of the eval batch norm behind it or None; then ReLU under relu."""
        import numpy as np
        x, weight = np.asarray(x), np.asarray(weight)
        norm = None if norm is None else [np.asarray(a) for a in norm]
        self._midas_f32("resnext_grouped_conv", [x, weight] + (norm or []))
        B, H, W, G, cg, Ho, Wo = resnext_check_grouped_conv(x.shape, weight.shape, stride, None if norm is None else [a.shape for a in norm],
                                                            eps)
        stride = _resnext_stride("resnext_grouped_conv", stride)
        out = np.zeros((B, G * cg, Ho, Wo), np.float32)
        with _DeviceArrays() as dev:
            dx, dw = dev.upload(np.ascontiguousarray(x)), dev.upload(np.ascontiguousarray(weight))
            dn = self._resnext_norm(dev, norm)
            do = dev.alloc(out.nbytes)
            self._check(self._fn("resnext_grouped_conv_device")(
                self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(G), C.c_int32(cg), C.c_int32(stride), dx, dw, dn,
                C.c_float(eps), C.c_int32(1 if relu else 0), do, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("resnext_grouped_conv: the device reported an error")
            dev.download(do, out)
        return out

    def resnext_conv(self, x, weight, stride=1, norm=None, eps=RESNEXT_EPS, relu=False, residual=None, split=0):
        """One dense convolution of the backbone, without bias (csrc/cvd_resnext.h): x [B, C, H, W] f32, weight [N, C, k, k] with
        (k, stride) in RESNEXT_DENSE_KERNELS, padding k // 2 -> [B, N, Ho, Wo]; the eval batch norm `norm` or None; ReLU under relu;
        with a residual max(residual + y, 0).  split: 0 = the rule (resnext_split), else the forced number of slices of K."""
        import numpy as np
        x, weight = np.asarray(x), np.asarray(weight)
        norm = None if norm is None else [np.asarray(a) for a in norm]
        residual = None if residual is None else np.asarray(residual)
        self._midas_f32("resnext_conv", [x, weight, residual] + (norm or []))
        B, H, W, Cin, N, k, Ho, Wo = resnext_check_conv(x.shape, weight.shape, stride, None if norm is None else [a.shape for a in norm],
                                                        eps, None if residual is None else residual.shape, split)
        stride = _resnext_stride("resnext_conv", stride)
        out = np.zeros((B, N, Ho, Wo), np.float32)
        with _DeviceArrays() as dev:
            dx, dw = dev.upload(np.ascontiguousarray(x)), dev.upload(np.ascontiguousarray(weight))
            dn = self._resnext_norm(dev, norm)
            dr = None if residual is None else dev.upload(np.ascontiguousarray(residual))
            do = dev.alloc(out.nbytes)
            self._check(self._fn("resnext_conv_device")(
                self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(Cin), C.c_int32(N), C.c_int32(k), C.c_int32(stride), dx, dw,
                dn, C.c_float(eps), C.c_int32(1 if relu else 0), dr, C.c_int32(split), do, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("resnext_conv: the device reported an error")
            dev.download(do, out)
        return out

    def resnext_maxpool(self, x):
        """nn.MaxPool2d(3, 2, 1) of x [B, C, H, W] f32 (csrc/cvd_resnext.h) -> [B, C, Ho, Wo]; padding counts as minus infinity."""
        import numpy as np
        x = np.asarray(x)
        self._midas_f32("resnext_maxpool", [x])
        B, Cn, H, W, Ho, Wo = resnext_check_maxpool(x.shape)
        out = np.zeros((B, Cn, Ho, Wo), np.float32)
        with _DeviceArrays() as dev:
            dx = dev.upload(np.ascontiguousarray(x))
            do = dev.alloc(out.nbytes)
            self._check(self._fn("resnext_maxpool_device")(self._h, C.c_int32(B), C.c_int32(Cn), C.c_int32(H), C.c_int32(W), dx, do, None))
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("resnext_maxpool: the device reported an error")
            dev.download(do, out)
        return out

    def _rxg_run(self, who, name, dev, scalars, tail, outs):
        """One `*_device` call of csrc/cvd_resnext_grad.h on uploaded arrays: scalars, then the device pointers `tail`, the null
        stream; downloads `outs` = [(device pointer, host array)]."""
        self._check(self._fn(name)(self._h, *scalars, *tail, None))
        if _hip_runtime().hipDeviceSynchronize() != 0:
            raise RuntimeError(f"{who}: the device reported an error")
        for d, a in outs:
            dev.download(d, a)

    def resnext_norm_train(self, c, norm, eps=RESNEXT_EPS, momentum=RESNEXT_MOMENTUM, training=True, relu=False, residual=None):
        """nn.BatchNorm2d on the raw convolution output c [B, N, H, W] f32 (csrc/cvd_resnext_grad.h); norm = (weight,
        bias, running_mean, running_var).  training: batch statistics, else the running ones.  y = (c - mean) invstd weight + bias,
        ReLU under relu, max(residual + y, 0) with a residual -> (y, save_mean, save_invstd, running_mean, running_var), the last
        two after the call (the inputs are not modified)."""
        import numpy as np
        c = np.asarray(c)
        norm = [np.asarray(a) for a in norm]
        residual = None if residual is None else np.asarray(residual)
        self._midas_f32("resnext_norm_train", [c, residual] + norm)
        B, N, H, W = resnext_check_norm_train(c.shape, [a.shape for a in norm], eps, momentum, training,
                                              None if residual is None else residual.shape)
        y = np.zeros((B, N, H, W), np.float32)
        vec = [np.zeros((N,), np.float32) for _ in range(4)]
        with _DeviceArrays() as dev:
            dc = dev.upload(np.ascontiguousarray(c))
            dn = [dev.upload(np.ascontiguousarray(a)) for a in norm]
            dr = None if residual is None else dev.upload(np.ascontiguousarray(residual))
            dm, di, dy = dev.alloc(4 * N), dev.alloc(4 * N), dev.alloc(y.nbytes)
            self._rxg_run("resnext_norm_train", "resnext_norm_train_device", dev,
                          [C.c_int32(B), C.c_int32(N), C.c_int32(H), C.c_int32(W)],
                          [dc, dn[0], dn[1], dn[2], dn[3], C.c_double(eps), C.c_double(momentum), C.c_int32(1 if training else 0),
                           C.c_int32(1 if relu else 0), dr, dm, di, dy],
                          [(dy, y), (dm, vec[0]), (di, vec[1]), (dn[2], vec[2]), (dn[3], vec[3])])
        return (y, *vec)

    def resnext_norm_grad(self, gy, c, mean, invstd, gamma, y=None, training=True, residual=False):
        """Backward of resnext_norm_train: gy, c [B, N, H, W] f32, the saved mean and invstd, the norm's weight; y = the layer's output
        where the forward applied a ReLU or the residual form (the mask is y > 0) -> (gc, g_gamma, g_beta, g_residual or None)."""
        import numpy as np
        gy, c, mean, invstd, gamma = (np.asarray(a) for a in (gy, c, mean, invstd, gamma))
        y = None if y is None else np.asarray(y)
        self._midas_f32("resnext_norm_grad", [gy, c, mean, invstd, gamma, y])
        B, N, H, W = resnext_check_norm_grad(gy.shape, c.shape, None if y is None else y.shape, [mean.shape, invstd.shape, gamma.shape],
                                             training)
        gc = np.zeros((B, N, H, W), np.float32)
        gg, gb = np.zeros((N,), np.float32), np.zeros((N,), np.float32)
        gr = np.zeros((B, N, H, W), np.float32) if residual else None
        with _DeviceArrays() as dev:
            dg, dc, dm, di, dw = (dev.upload(np.ascontiguousarray(a)) for a in (gy, c, mean, invstd, gamma))
            dy = None if y is None else dev.upload(np.ascontiguousarray(y))
            do, dgg, dgb = dev.alloc(gc.nbytes), dev.alloc(4 * N), dev.alloc(4 * N)
            dr = dev.alloc(gc.nbytes) if residual else None
            self._rxg_run("resnext_norm_grad", "resnext_norm_grad_device", dev, [C.c_int32(B), C.c_int32(N), C.c_int32(H), C.c_int32(W)],
                          [dg, dc, dy, dm, di, dw, C.c_int32(1 if training else 0), do, dgg, dgb, dr],
                          [(do, gc), (dgg, gg), (dgb, gb)] + ([(dr, gr)] if residual else []))
        return gc, gg, gb, gr

    def resnext_grouped_conv_grad_input(self, gy, weight, x_size, stride=1):
        """Input gradient of resnext_grouped_conv: gy [B, G Cg, Ho, Wo] f32, weight [G Cg, Cg, 3, 3], x_size = (H, W) of the
        convolution's input -> gx [B, G Cg, H, W]."""
        import numpy as np
        gy, weight = np.asarray(gy), np.asarray(weight)
        self._midas_f32("resnext_grouped_conv_grad_input", [gy, weight])
        B, H, W, G, cg = resnext_check_grouped_conv_grad_input(gy.shape, weight.shape, x_size, stride)
        stride = _resnext_stride("resnext_grouped_conv_grad_input", stride)
        gx = np.zeros((B, G * cg, H, W), np.float32)
        with _DeviceArrays() as dev:
            dg, dw = dev.upload(np.ascontiguousarray(gy)), dev.upload(np.ascontiguousarray(weight))
            do = dev.alloc(gx.nbytes)
            self._rxg_run("resnext_grouped_conv_grad_input", "resnext_grouped_conv_grad_input_device", dev,
                          [C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(G), C.c_int32(cg), C.c_int32(stride)], [dg, dw, do],
                          [(do, gx)])
        return gx

    def resnext_grouped_conv_grad_weight(self, gy, x, channels_per_group, stride=1, split=0):
        """Weight gradient of resnext_grouped_conv: gy [B, G Cg, Ho, Wo] f32, x [B, G Cg, H, W] -> gW [G Cg, Cg, 3, 3].  split: 0 =
        the rule (resnext_wgrad_split), else the forced number of slices of the pixels."""
        import numpy as np
        gy, x = np.asarray(gy), np.asarray(x)
        self._midas_f32("resnext_grouped_conv_grad_weight", [gy, x])
        B, H, W, G, cg = resnext_check_grouped_conv_grad_weight(gy.shape, x.shape, channels_per_group, stride, split)
        stride = _resnext_stride("resnext_grouped_conv_grad_weight", stride)
        gw = np.zeros((G * cg, cg, 3, 3), np.float32)
        with _DeviceArrays() as dev:
            dg, dx = dev.upload(np.ascontiguousarray(gy)), dev.upload(np.ascontiguousarray(x))
            do = dev.alloc(gw.nbytes)
            self._rxg_run("resnext_grouped_conv_grad_weight", "resnext_grouped_conv_grad_weight_device", dev,
                          [C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(G), C.c_int32(cg), C.c_int32(stride)],
                          [dg, dx, C.c_int32(split), do], [(do, gw)])
        return gw

    def resnext_conv_grad_input(self, gy, weight, x_size, stride=1, add=None):
        """Input gradient of a 1 x 1 convolution of resnext_conv at stride 1 or 2: gy [B, N, Ho, Wo] f32, weight [N, C, 1, 1], x_size =
        (H, W) -> gx [B, C, H, W] = conv_transpose(gy) + add."""
        import numpy as np
        gy, weight = np.asarray(gy), np.asarray(weight)
        add = None if add is None else np.asarray(add)
        self._midas_f32("resnext_conv_grad_input", [gy, weight, add])
        B, H, W, Cin, N = resnext_check_conv_grad_input(gy.shape, weight.shape, x_size, stride, None if add is None else add.shape)
        stride = _resnext_stride("resnext_conv_grad_input", stride)
        gx = np.zeros((B, Cin, H, W), np.float32)
        with _DeviceArrays() as dev:
            dg, dw = dev.upload(np.ascontiguousarray(gy)), dev.upload(np.ascontiguousarray(weight))
            da = None if add is None else dev.upload(np.ascontiguousarray(add))
            do = dev.alloc(gx.nbytes)
            self._rxg_run("resnext_conv_grad_input", "resnext_conv_grad_input_device", dev,
                          [C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(Cin), C.c_int32(N), C.c_int32(1), C.c_int32(stride)],
                          [dg, dw, da, do], [(do, gx)])
        return gx

    def resnext_conv_grad_weight(self, gy, x, kernel_size, stride=1, split=0):
        """Weight gradient of a dense convolution of resnext_conv: gy [B, N, Ho, Wo] f32, x [B, C, H, W], (kernel_size, stride) in
        RESNEXT_DENSE_KERNELS -> gW [N, C, k, k]."""
        import numpy as np
        gy, x = np.asarray(gy), np.asarray(x)
        self._midas_f32("resnext_conv_grad_weight", [gy, x])
        B, H, W, Cin, N, k = resnext_check_conv_grad_weight(gy.shape, x.shape, kernel_size, stride, split)
        stride = _resnext_stride("resnext_conv_grad_weight", stride)
        gw = np.zeros((N, Cin, k, k), np.float32)
        with _DeviceArrays() as dev:
            dg, dx = dev.upload(np.ascontiguousarray(gy)), dev.upload(np.ascontiguousarray(x))
            do = dev.alloc(gw.nbytes)
            self._rxg_run("resnext_conv_grad_weight", "resnext_conv_grad_weight_device", dev,
                          [C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(Cin), C.c_int32(N), C.c_int32(k), C.c_int32(stride)],
                          [dg, dx, C.c_int32(split), do], [(do, gw)])
        return gw

    def resnext_maxpool_grad(self, x, gy):
        """Backward of resnext_maxpool: x [B, C, H, W] f32 its input, gy [B, C, Ho, Wo] -> gx [B, C, H, W]; a window's gradient goes to
        its first maximum in row-major order, as torch's."""
        import numpy as np
        x, gy = np.asarray(x), np.asarray(gy)
        self._midas_f32("resnext_maxpool_grad", [x, gy])
        B, Cn, H, W = resnext_check_maxpool_grad(x.shape, gy.shape)
        gx = np.zeros((B, Cn, H, W), np.float32)
        with _DeviceArrays() as dev:
            dx, dg = dev.upload(np.ascontiguousarray(x)), dev.upload(np.ascontiguousarray(gy))
            do = dev.alloc(gx.nbytes)
            self._rxg_run("resnext_maxpool_grad", "resnext_maxpool_grad_device", dev,
                          [C.c_int32(B), C.c_int32(Cn), C.c_int32(H), C.c_int32(W)], [dx, dg, do], [(do, gx)])
        return gx

    def resnext_block_train(self, x, weights, norms, stride=1, eps=RESNEXT_EPS, momentum=RESNEXT_MOMENTUM, training=True):
        """One Bottleneck in training form, ONE library call (cvd_resnext_block_train_device): x [B, C, H, W] f32, weights = conv1,
        conv2, conv3 (and downsample.0), norms = (weight, bias, running_mean, running_var) per convolution, training = one flag or
        one per norm -> (out, saved, running): the block's output, the saved table (resnext_block_saved_shapes; saved[11] is out)
        and the (running_mean, running_var) per norm after the call.  The inputs are not modified."""
        import numpy as np
        x = np.asarray(x)
        weights = [np.asarray(a) for a in weights]
        norms = [[np.asarray(a) for a in four] for four in norms]
        self._midas_f32("resnext_block_train", [x] + weights + [a for four in norms for a in four])
        B, H, W, Cin, width, out, G, stride, down, flags = resnext_check_block(
            x.shape, [a.shape for a in weights], [[a.shape for a in four] for four in norms], stride, eps, momentum, training)
        n = len(weights)
        saved = [np.zeros(s, np.float32) for s in resnext_block_saved_shapes(B, H, W, Cin, width, out, stride, down)]
        with _DeviceArrays() as dev:
            dx = dev.upload(np.ascontiguousarray(x))
            dw = (C.c_void_p * n)(*[dev.upload(np.ascontiguousarray(a)).value for a in weights])
            dn = [dev.upload(np.ascontiguousarray(a)) for four in norms for a in four]
            ds = [dev.alloc(a.nbytes) for a in saved]
            running = [[np.zeros_like(four[2]), np.zeros_like(four[3])] for four in norms]
            self._rxg_run("resnext_block_train", "resnext_block_train_device", dev,
                          [C.c_int32(v) for v in (B, H, W, Cin, width, out, G, stride, int(down))],
                          [dx, dw, (C.c_void_p * (4 * n))(*[d.value for d in dn]), C.c_double(eps), C.c_double(momentum),
                           (C.c_int32 * n)(*[int(f) for f in flags]), (C.c_void_p * (4 * n))(*[d.value for d in ds])],
                          list(zip(ds, saved)) + [(dn[4 * i + 2 + j], running[i][j]) for i in range(n) for j in range(2)])
        return saved[11], saved, running

    def resnext_block_backward(self, gy, x, weights, gammas, saved, stride=1, training=True, input_gradient=True):
        """Backward of resnext_block_train, ONE library call (cvd_resnext_block_backward_device): gy of the output's shape, the
        block's input, weights, the norms' weights and the saved table -> (gx or None, [gW], [g_gamma], [g_beta])."""
        import numpy as np
        gy, x = np.asarray(gy), np.asarray(x)
        weights, gammas, saved = ([np.asarray(a) for a in v] for v in (weights, gammas, saved))
        self._midas_f32("resnext_block_backward", [gy, x] + weights + gammas + saved)
        fake = [[g.shape] * 4 for g in gammas]
        B, H, W, Cin, width, out, G, stride, down, flags = resnext_check_block(x.shape, [a.shape for a in weights], fake, stride,
                                                                               training=training)
        shapes = resnext_block_saved_shapes(B, H, W, Cin, width, out, stride, down)
        if [a.shape for a in saved] != shapes or gy.shape != shapes[11]:
            raise ValueError(f"resnext_block_backward: the saved table must be {shapes} and gy {shapes[11]}")
        n = len(weights)
        gx = np.zeros(x.shape, np.float32) if input_gradient else None
        gw = [np.zeros(a.shape, np.float32) for a in weights]
        gg, gb = ([np.zeros(a.shape, np.float32) for a in gammas] for _ in range(2))
        with _DeviceArrays() as dev:
            table = lambda arrays: (C.c_void_p * len(arrays))(*[dev.upload(np.ascontiguousarray(a)).value for a in arrays])
            dgy, dx = dev.upload(np.ascontiguousarray(gy)), dev.upload(np.ascontiguousarray(x))
            dgx = dev.alloc(gx.nbytes) if input_gradient else None
            outs = [[dev.alloc(a.nbytes) for a in group] for group in (gw, gg, gb)]
            self._rxg_run("resnext_block_backward", "resnext_block_backward_device", dev,
                          [C.c_int32(v) for v in (B, H, W, Cin, width, out, G, stride, int(down))],
                          [dgy, dx, table(weights), table(gammas), table(saved), (C.c_int32 * n)(*[int(f) for f in flags]), dgx]
                          + [(C.c_void_p * n)(*[d.value for d in group]) for group in outs],
                          ([(dgx, gx)] if input_gradient else []) + [(d, a) for group, arrays in zip(outs, (gw, gg, gb))
                                                                     for d, a in zip(group, arrays)])
        return gx, gw, gg, gb

    def midas_backbone(self, images, weights, norms, blocks=RESNEXT101_32X8D[0], groups=RESNEXT101_32X8D[1],
                       width_per_group=RESNEXT101_32X8D[2], eps=RESNEXT_EPS, kernel_ms=None):
        """ResNet(Bottleneck, blocks, groups, width_per_group).forward up to layer4 in eval mode: images [B, 3, H, W]
        f32 with sides that are multiples of 32, weights / norms = one weight and (weight, bias, running_mean, running_var) per
        convolution of resnext_conv_table -> the four stages' outputs.  kernel_ms (measurement): a list that receives the per-launch
        milliseconds of cvd_midas_backbone_timed (2 per convolution, then the pool)."""
        import numpy as np
        images = np.asarray(images)
        weights = [np.asarray(a) for a in weights]
        norms = [[np.asarray(a) for a in four] for four in norms]
        self._midas_f32("midas_backbone", [images] + weights + [a for four in norms for a in four])
        B, H, W, table, out_shapes = resnext_check_backbone(images.shape, blocks, groups, width_per_group, [a.shape for a in weights],
                                                            [[a.shape for a in four] for four in norms], eps)
        outs = [np.zeros(s, np.float32) for s in out_shapes]
        n = len(table)
        with _DeviceArrays() as dev:
            di = dev.upload(np.ascontiguousarray(images))
            dw = (C.c_void_p * n)(*[dev.upload(np.ascontiguousarray(a)).value for a in weights])
            dn = (C.c_void_p * (4 * n))(*[dev.upload(np.ascontiguousarray(a)).value for four in norms for a in four])
            douts = [dev.alloc(o.nbytes) for o in outs]
            do = (C.c_void_p * 4)(*[d.value for d in douts])
            args = (self._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), (C.c_int32 * 4)(*[int(b) for b in blocks]), C.c_int32(groups),
                    C.c_int32(width_per_group), C.c_float(eps), di, dw, dn, do, None)
            if kernel_ms is None:
                self._check(self._fn("midas_backbone_device")(*args))
            else:
                ms = (C.c_double * (2 * n + 1))()
                self._check(self._fn("midas_backbone_timed")(*args, ms))
                kernel_ms[:] = list(ms)
            if _hip_runtime().hipDeviceSynchronize() != 0:
                raise RuntimeError("midas_backbone: the device reported an error")
            for d, o in zip(douts, outs):
                dev.download(d, o)
        return outs

    def num_active_constraints(self):
        return int(self._lib.cvd_num_active_constraints(self._h))

    def block_inverse_debug(self, blocks, variant=0):
        """f32 inverses of SPD f64 blocks [n, B, B] through the block-Jacobi kernel (variant 0 MFMA blocked sweep = the
        default path, 1 scalar sweep, 2 LDS Cholesky) and the number of failed pivots."""
        import numpy as np
        a = np.ascontiguousarray(blocks, dtype=np.float64)
        n, B, B2 = a.shape
        assert B == B2
        out = np.zeros((n, B, B), dtype=np.float32)
        fl = C.c_int32(0)
        self._check(self._fn("block_inverse_debug")(self._h, C.c_int32(n), C.c_int32(B), a.ctypes.data_as(C.POINTER(C.c_double)),
                                                    C.c_int32(variant), out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(fl)))
        return out, fl.value

    def dense_inverse_debug(self, a):
        """f64 inverse of one dense SPD f64 matrix [n, n] through the dense coarse level's kernel (k_dense_spd_inverse) and
        its failure word (1: non-positive pivot, bit 30: barrier timeout)."""
        import numpy as np
        a = np.ascontiguousarray(a, dtype=np.float64)
        n = a.shape[0]
        assert a.shape == (n, n)
        out = np.zeros((n, n), dtype=np.float64)
        fl = C.c_int32(0)
        self._check(self._fn("dense_inverse_debug")(self._h, C.c_int32(n), a.ctypes.data_as(C.POINTER(C.c_double)),
                                                    out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(fl)))
        return out, fl.value

    def temporal_debug(self):
        """Third preconditioner level after the last solve: None when it was off, else its dimensions, Galerkin matrix, the inverse
        in use and the damping vector of the last LM iteration."""
        import numpy as np
        dims = (C.c_int32 * 6)()
        self._check(self._fn("temporal_debug")(self._h, dims, None, None, None, None))
        if dims[0] == 0:
            return None
        n = dims[0]
        a = np.zeros((n, n))
        ai = np.zeros((n, n))
        lam = np.zeros(self.num_frames * self.block_size())
        fl = C.c_int32(0)
        dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
        self._check(self._fn("temporal_debug")(self._h, dims, dp(a), dp(ai), dp(lam), C.byref(fl)))
        return {"NT": n, "S": dims[1], "nn": dims[2], "step": dims[3], "Sx": dims[4], "Sy": dims[5], "a_t": a, "a_t_inverse": ai,
                "lam": lam, "failed": fl.value}

    def path_info(self):
        """Which variant of the linear solver the last solve ran (cvd_path_info)."""
        out = (C.c_int32 * 8)()
        self._check(self._fn("path_info")(self._h, out))
        form = {-1: "none", 0: "exact sparse factor", 1: "exact dense inverse", 2: "temporal pose level"}[out[1]]
        return {"pose_graph_level": form, "depth_grid_level": bool(out[2]), "fused_tail": bool(out[3] & 1), "tail_rows_staged": bool(out[3] & 2),
                # (the next product sums the tail's r^T z shares; how many there were)
                "product_sums_shares": bool(out[3] & 4), "rz_shares": out[3] >> 8,
                "tail_disabled": bool(out[4]),
                "taps": out[5], "work_items": out[6], "cross_blocks": bool(out[7])}

    def product_launch_debug(self):
        """The handle's last product launch (cvd_product_launch_debug): workgroup size, kernel variant, work items, CUs counted."""
        out = (C.c_int32 * 6)()
        self._check(self._fn("product_launch_debug")(self._h, out))
        kind = {-1: "none", 0: "generic list", 1: "fast list", 2: "fast dense", 3: "cross blocks"}[out[3]]
        return {"threads": out[0], "spec": out[1], "kd": out[2], "kind": out[3], "kind_name": kind, "work_items": out[4],
                "num_cu": out[5]}

    def assembly_launch_debug(self):
        """The handle's last assembly launch (cvd_assembly_launch_debug): workgroup size, kernel variant, workgroups, parts of split
        frames, staging rows per wave and segments of the segment walk (stage_depth -1: a unit loop ran), and the per-frame costs it wrote
        (their sum is the cost of the evaluation)."""
        import numpy as np
        out = (C.c_int32 * 8)()
        cost = np.zeros(self.num_frames, dtype=np.float64)
        self._check(self._fn("assembly_launch_debug")(self._h, out, cost.ctypes.data_as(C.POINTER(C.c_double))))
        kind = {-1: "none", 0: "generic", 1: "fast list", 2: "fast dense", 3: "dense fold"}[out[3]]
        return {"threads": out[0], "spec": out[1], "kd": out[2], "kind": out[3], "kind_name": kind, "workgroups": out[4],
                "split_parts": out[5], "stage_depth": out[6], "segments": out[7], "cost_frame": cost}

    def coarse_debug(self):
        """(A_c, A_c^-1 as applied, pivot failures) of the coarse preconditioner level after the last solve."""
        import numpy as np
        n = C.c_int32(0)
        self._check(self._fn("coarse_debug")(self._h, C.byref(n), None, None, None))
        if n.value == 0:
            return None
        a = np.zeros((n.value, n.value))
        ai = np.zeros((n.value, n.value))
        fl = C.c_int32(0)
        self._check(self._fn("coarse_debug")(self._h, C.byref(n), a.ctypes.data_as(C.POINTER(C.c_double)),
                                             ai.ctypes.data_as(C.POINTER(C.c_double)), C.byref(fl)))
        return {"a_c": a, "a_c_inverse": ai, "failed": fl.value}
