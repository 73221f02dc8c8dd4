"""Flow consistency masks and pair statistics from dataset files: the drop-in for the reference's Flow.compute_flow_masks
(flow.py:180-209) and Flow.compute_flow_pair_stats (flow.py:44-74), i.e. everything its Flow class leaves on disk after RAFT.
The masks are computed on the GPU (Solver.flow_consistency_masks, csrc/cvd_flowmask.h); files are read and
written with numpy and Pillow (no torch, no cv2).
"""
import json
import os
import re

import numpy as np

from .dataset_io import read_raw_image

_FLOW_NAME = re.compile(r"^flow_(\d+)_(\d+)\.raw$")
# kept-pixel counts of the masks this process wrote: {real base_dir: {(a, b): (pixels set, pixels)}}; compute_flow_pair_stats
# takes its ratios from here and reads only the other masks back from their PNGs
_KEPT = {}

DEFAULT_MAX_BATCH_BYTES = 256 << 20


def _flow_path(base_dir, a, b):
    return os.path.join(base_dir, "flow", f"flow_{a:06d}_{b:06d}.raw")


def _mask_path(base_dir, a, b):
    return os.path.join(base_dir, "flow_mask", f"mask_{a:06d}_{b:06d}.png")


def _color_path(base_dir, i):
    return os.path.join(base_dir, "color_down", f"frame_{i:06d}.raw")


def _read(path, what):
    if not os.path.isfile(path):
        raise FileNotFoundError(f"flow masks: {what} {path} does not exist")
    return read_raw_image(path)


def compute_flow_masks(base_dir, flow_thresh=1, color_thresh=1, device=0, max_batch_bytes=DEFAULT_MAX_BATCH_BYTES):
    """For every flow/flow_%06d_%06d.raw of `base_dir` whose flow_mask/mask_%06d_%06d.png does not exist yet, compute and
    write the masks of BOTH directions of that pair (as the reference does); a pair and its reverse are handled once, and a
    pair whose two masks exist is left alone.  Returns the number of mask files written.

    The pairs are processed in batches of at most `max_batch_bytes` of flow data (both directions); every batch loads each
    colour frame its pairs name once.  The default, 256 MiB, holds 195 pairs at 384 x 224: large enough that the launch and
    the copies are amortised over many pairs and that the ~14 pairs a frame takes part in (hierarchical pair lists, sorted
    here by frame) mostly share one load of its colour image, small enough that the host staging arrays and the device
    buffers (flows, masks and colour table, about 1.2 x the flow bytes) stay far below the memory of either side.

    A missing reverse flow or colour frame raises FileNotFoundError, an image of another size ValueError; both name the file."""
    from PIL import Image
    from .api import Solver
    if max_batch_bytes < 1:
        raise ValueError(f"max_batch_bytes must be >= 1 (got {max_batch_bytes})")
    flow_dir = os.path.join(base_dir, "flow")
    todo = set()
    for name in os.listdir(flow_dir):
        m = _FLOW_NAME.match(name)
        if not m:
            continue
        a, b = int(m.group(1)), int(m.group(2))
        if a != b and not os.path.isfile(_mask_path(base_dir, a, b)):
            todo.add((min(a, b), max(a, b)))
    if not todo:
        return 0
    todo = sorted(todo)
    for a, b in todo:  # every input must exist before any work
        for path, what in ((_flow_path(base_dir, a, b), "flow"), (_flow_path(base_dir, b, a), "reverse flow"),
                           (_color_path(base_dir, a), "colour frame"), (_color_path(base_dir, b), "colour frame")):
            if not os.path.isfile(path):
                raise FileNotFoundError(f"flow masks: {what} {path} does not exist")
    os.makedirs(os.path.join(base_dir, "flow_mask"), exist_ok=True)
    first = _read(_flow_path(base_dir, *todo[0]), "flow")
    if first.ndim != 3 or first.shape[2] != 2:
        raise ValueError(f"flow masks: {_flow_path(base_dir, *todo[0])} is not a 2-channel flow image (shape {first.shape})")
    H, W = first.shape[:2]
    per_batch = max(1, int(max_batch_bytes) // (2 * H * W * 8))
    kept_cache = _KEPT.setdefault(os.path.realpath(base_dir), {})
    written = 0
    solver = Solver(device)
    try:
        for start in range(0, len(todo), per_batch):
            pairs = todo[start:start + per_batch]
            frames = sorted({f for p in pairs for f in p})
            slot = {f: i for i, f in enumerate(frames)}
            color = None
            for f in frames:
                img = _read(_color_path(base_dir, f), "colour frame")
                img = img[..., None] if img.ndim == 2 else img
                if color is None:
                    if img.shape[:2] != (H, W) or not 1 <= img.shape[2] <= 4:
                        raise ValueError(f"flow masks: {_color_path(base_dir, f)} has shape {img.shape}, the flows are {H} x {W}")
                    color = np.zeros((len(frames), H, W, img.shape[2]), np.float32)
                if img.shape != color.shape[1:]:
                    raise ValueError(f"flow masks: {_color_path(base_dir, f)} has shape {img.shape}, expected {color.shape[1:]}")
                color[slot[f]] = img
            flow_ab = np.zeros((len(pairs), H, W, 2), np.float32)
            flow_ba = np.zeros((len(pairs), H, W, 2), np.float32)
            for i, (a, b) in enumerate(pairs):
                for dst, path in ((flow_ab, _flow_path(base_dir, a, b)), (flow_ba, _flow_path(base_dir, b, a))):
                    fl = _read(path, "flow")
                    if fl.shape != (H, W, 2):
                        raise ValueError(f"flow masks: {path} has shape {fl.shape}, expected {(H, W, 2)}")
                    dst[i] = fl
            index = np.array([[slot[a], slot[b]] for a, b in pairs], np.int32)
            mask_ab, mask_ba, kept = solver.flow_consistency_masks(color, index, flow_ab, flow_ba, flow_thresh, color_thresh)
            for i, (a, b) in enumerate(pairs):
                for (x, y), mk, k in (((a, b), mask_ab[i], kept[i, 0]), ((b, a), mask_ba[i], kept[i, 1])):
                    # (zlib level 1, cv2.imwrite's default too: a 0 / 255 image gains little from more, and the encoder is
                    # the largest share of this function's time once the flows are in the page cache)
                    Image.fromarray(mk, "L").save(_mask_path(base_dir, x, y), compress_level=1)
                    kept_cache[(x, y)] = (int(k), H * W)
                    written += 1
    finally:
        solver.close()
    return written


def _mask_ratio(base_dir, a, b):
    cached = _KEPT.get(os.path.realpath(base_dir), {}).get((a, b))
    if cached is not None:
        return cached[0] / cached[1]
    from PIL import Image
    path = _mask_path(base_dir, a, b)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"flow pair stats: mask {path} does not exist")
    mask = np.asarray(Image.open(path).convert("L"))
    return int(np.sum(mask > 0)) / int(mask.shape[0] * mask.shape[1])


def compute_flow_pair_stats(base_dir, frame_pairs):
    """<base_dir>/flow_list.json as the reference writes it: [["frame0", "frame1", "mask_ratio"], [a, b, r], [b, a, r], ...] in
    the order of `frame_pairs` (a pair and its reverse handled once), r = the smaller of the two directions' shares of kept
    pixels, a double.  When the file exists it is left alone.  The counts come from the masks compute_flow_masks wrote in this
    process, else from the PNGs.  Returns the file's path."""
    path = os.path.join(base_dir, "flow_list.json")
    if os.path.isfile(path):
        return path
    results = [["frame0", "frame1", "mask_ratio"]]
    checked = set()
    for pair in frame_pairs:
        a, b = int(pair[0]), int(pair[1])
        if (a, b) in checked:
            continue
        checked.update(((a, b), (b, a)))
        r = min(_mask_ratio(base_dir, a, b), _mask_ratio(base_dir, b, a))
        results.append([a, b, r])
        results.append([b, a, r])
    with open(path, "w") as f:
        json.dump(results, f)
    return path
