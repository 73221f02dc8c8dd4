"""Child process of tests/test_gpu_sceneflow.py::test_torch_module (python -m tests.sceneflow_torch_child <dtype>): torch is
imported first, then the library; robust_cvd_amd.scene_flow.SceneFlowLoss on GPU tensors against the array path
(Solver.scene_flow_loss) on the same inputs, with N = 6 (all terms) and N = 2 (the static term alone)."""
import sys
import types

import numpy as np
import torch

from robust_cvd_amd import api
from robust_cvd_amd.scene_flow import SceneFlowLoss
from tests import margins
from tests import sceneflow_cases as sc
from tests import sceneflow_reference as sr

EPS32 = 2.0 ** -23


def options(combo):
    lam = combo[5]
    return types.SimpleNamespace(distance_type_static=combo[1], distance_type_smooth=combo[2], distance_scale=combo[3],
                                 distance_alpha=combo[4], lambda_scene_flow_static=lam[0], lambda_smooth_reprojection=lam[1],
                                 lambda_smooth_disparity=lam[2], lambda_smooth_depth_ratio=lam[3], recon="i3d")


def check_torch_module(solver, golden, dtype, combo, N):
    """SceneFlowLoss(opt)(depths, metadata) on GPU tensors of the reference's layout: the array path's values bit for bit, and
    (3 loss).backward() leaves three times the array path's gradient (the same kernels: within the repeatability bars)."""
    case = sc.make_case(combo[0])
    npdt = np.dtype(dtype)
    td = getattr(torch, dtype)
    B, H, W = case["P"], case["H"], case["W"]
    assert case["F"] == B * N
    ref = solver.scene_flow_loss(**sc.case_kwargs(case, npdt), **sc.combo_kwargs(combo), grad=True, maps=True)
    total, terms, g, maps = ref
    dev = torch.device("cuda", 0)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=td, device=dev)
    warp = t(case["warp_norm"]).view(B, N, 2, H, W)
    warp_before = warp.clone()
    meta = {"extrinsics": t(case["extrinsics"]).view(B, N, 3, 4), "intrinsics": t(case["intrinsics"]).view(B, N, 4), "warp": warp,
            "geometry_consistency": {"flows": tuple(t(f) for f in case["flows"]),
                                     "masks": tuple(t(m).view(B, 1, H, W) for m in case["masks"])}}
    if N == 6:
        meta["temporal_smoothness"] = {"flows": tuple(t(f) for f in case["nflows"]),
                                       "masks": tuple(t(m).view(B, 1, H, W) for m in case["nmasks"]),
                                       "valid": t(case["valid"]).view(B, 2, 1)}
    module = SceneFlowLoss(options(combo))
    depths = t(case["depth"]).view(B, N, H, W).requires_grad_(True)
    loss, batch, scene_flow = module(depths, meta)
    assert scene_flow is None      # no device -> host copy unless asked for
    assert loss.dtype == td and loss.shape == () and loss.requires_grad
    want = {name for q, name in enumerate(sr.TERMS) if combo[5][q] > 0}
    assert set(batch) == want and all(v.shape == (B,) and not v.requires_grad for v in batch.values())
    # the same kernels on the same inputs: the forward repeats bit for bit (rounded to the tensors' dtype)
    assert float(loss) == float(npdt.type(total))
    for name in want:
        assert np.array_equal(batch[name].cpu().numpy(), terms[name].astype(npdt))
    (3 * loss).backward()
    bar = margins.limit(1e-9 if dtype == "float64" else 64 * EPS32, 1e-15 if dtype == "float64" else EPS32)
    got = depths.grad.cpu().numpy().reshape(g.shape).astype(np.float64)
    margins.below(f"sf torch gradient {dtype} N={N}", np.abs(got - 3.0 * g).max() / np.abs(3.0 * g).max(), bar)
    assert torch.equal(warp, warp_before)      # not scaled in place
    # the maps on request: the reference's list, as numpy, in its order
    with_maps = SceneFlowLoss(options(combo), scene_flow_maps=True)
    with torch.no_grad():
        loss3, _batch, scene_flow = with_maps(depths.detach(), meta)
    assert float(loss3) == float(loss) and not loss3.requires_grad
    assert isinstance(scene_flow, list) and len(scene_flow) == (6 if N == 6 else 2)
    for k, m in enumerate(scene_flow):
        assert isinstance(m, np.ndarray) and m.shape == (B, 3, H, W) and np.array_equal(m, maps[k])
    try:
        module(depths.detach().cpu(), meta)
    except ValueError as e:
        assert "GPU" in str(e)
    else:
        raise AssertionError("a CPU tensor was accepted")


def check_bad_frame_index(solver, dtype):
    """The device entry point cannot check the frame tables before the launch: a neighbour outside [0, F) is never dereferenced
    and the total comes back NaN."""
    case = sc.make_case("batch")
    td = getattr(torch, dtype)
    dev = torch.device("cuda", 0)
    B, H, W = case["P"], case["H"], case["W"]
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=td, device=dev)
    module = SceneFlowLoss(options(sc.COMBOS[11]))
    module._frames[(B, 6, dev)] = (torch.tensor(case["pairs"], device=dev), torch.tensor([[2, 3, 4, 5], [8, 9, 10, 12]],
                                                                                         dtype=torch.int32, device=dev))
    meta = {"extrinsics": t(case["extrinsics"]).view(B, 6, 3, 4), "intrinsics": t(case["intrinsics"]).view(B, 6, 4),
            "warp": t(case["warp_norm"]).view(B, 6, 2, H, W),
            "temporal_smoothness": {"flows": tuple(t(f) for f in case["nflows"]),
                                    "masks": tuple(t(m).view(B, 1, H, W) for m in case["nmasks"]),
                                    "valid": torch.ones(B, 2, 1, dtype=td, device=dev)}}
    depths = t(case["depth"]).view(B, 6, H, W).requires_grad_(True)
    loss, batch, _ = module(depths, meta)
    assert torch.isnan(loss) and not torch.isnan(batch["smooth_reproj"][0]) and torch.isnan(batch["smooth_reproj"][1])
    loss.backward()
    # the anchor with the bad neighbour added nothing: its own frame and its other neighbour stay at zero
    assert torch.isfinite(depths.grad).all() and not depths.grad[1, 1].any() and not depths.grad[1, 4].any()
    assert depths.grad[1, 0].any() and depths.grad[0].any()


def check_misaligned_tables(golden, dtype):
    """Tables that are not aligned to four elements take the one-pixel-per-thread kernels (case `batch`: 2 x 6 frames of 16 x 24,
    two workgroups per image where the aligned run has one): depths, and in a second run one neighbour flow tensor, as
    contiguous views offset by one element.  Total, terms and gradient against the fixture with the bars of
    test_gpu_sceneflow.py for this combination: f64 1e-10 relative and the gradient 1e-9 x max |g|; f32 total and gradient 8 x
    the reference's own f32 delta (never below 2^-23; that test sets no f32 bar for the terms, so they are checked in f64)."""
    combo = sc.COMBOS[10]
    key, case = sc.combo_key(combo), sc.make_case("batch")
    td = getattr(torch, dtype)
    B, H, W = case["P"], case["H"], case["W"]
    assert W % 4 == 0 and case["F"] == 6 * B and all(v > 0 for v in combo[5])
    dev = torch.device("cuda", 0)
    ref_total, ref_terms, ref_g = float(golden[f"{key}/total"]), golden[f"{key}/terms"], golden[f"{key}/grad"]
    d_total, d_grad = float(golden[f"{key}/delta_total"]), float(golden[f"{key}/delta_grad"])
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=td, device=dev)

    def shifted(a):
        flat = torch.zeros(a.size + 1, dtype=td, device=dev)
        flat[1:] = t(a).ravel()
        v = flat[1:].view(a.shape)
        assert v.is_contiguous() and v.data_ptr() % (4 * v.element_size()) != 0
        return v
    for which in ("depths", "flow"):
        depths = (shifted if which == "depths" else t)(case["depth"]).view(B, 6, H, W).detach().requires_grad_(True)
        assert (depths.data_ptr() % (4 * depths.element_size()) != 0) == (which == "depths")
        nflows = [t(f) for f in case["nflows"]]
        if which == "flow":
            nflows[2] = shifted(case["nflows"][2])
        meta = {"extrinsics": t(case["extrinsics"]).view(B, 6, 3, 4), "intrinsics": t(case["intrinsics"]).view(B, 6, 4),
                "warp": t(case["warp_norm"]).view(B, 6, 2, H, W),
                "geometry_consistency": {"flows": tuple(t(f) for f in case["flows"]),
                                         "masks": tuple(t(m).view(B, 1, H, W) for m in case["masks"])},
                "temporal_smoothness": {"flows": tuple(nflows), "masks": tuple(t(m).view(B, 1, H, W) for m in case["nmasks"]),
                                        "valid": t(case["valid"]).view(B, 2, 1)}}
        loss, batch, _ = SceneFlowLoss(options(combo))(depths, meta)
        loss.backward()
        g = depths.grad.cpu().numpy().reshape(ref_g.shape).astype(np.float64)
        what = f"sf misaligned {which} {dtype}"
        f64 = dtype == "float64"
        margins.below(f"{what} total", abs(float(loss) - ref_total) / abs(ref_total), 1e-10 if f64 else 8 * max(d_total, EPS32))
        margins.below(f"{what} grad", np.abs(g - ref_g).max() / np.abs(ref_g).max(), 1e-9 if f64 else 8 * max(d_grad, EPS32))
        if f64:
            tt = np.stack([batch[name].cpu().numpy() for name in sr.TERMS], 1)
            margins.below(f"{what} terms", np.max(np.abs(tt - ref_terms) / np.abs(ref_terms)), 1e-10)


if __name__ == "__main__":
    torch.cuda.init()
    s = api.Solver(0)
    golden = np.load(sr.GOLDEN)
    check_torch_module(s, golden, sys.argv[1], sc.COMBOS[10], 6)
    check_torch_module(s, golden, sys.argv[1], sc.COMBOS[12], 2)
    check_bad_frame_index(s, sys.argv[1])
    check_misaligned_tables(golden, sys.argv[1])
    s.close()
    print("torch module ok")
