"""Child process of tests/test_gpu_consistency.py::test_torch_module (python -m tests.consistency_torch_child <dtype>): torch is
imported first, then the library; robust_cvd_amd.consistency.ConsistencyLoss on GPU tensors against the array path
(Solver.consistency_loss) on the same inputs."""
import sys
import types

import numpy as np
import torch

from robust_cvd_amd import api
from robust_cvd_amd.consistency import ConsistencyLoss
from tests import consistency_cases as cc
from tests import consistency_reference as cr
from tests import margins

EPS32 = 2.0 ** -23


def run(solver, combo, dtype):
    case = cc.make_case(combo[0])
    return solver.consistency_loss(*cc.case_args(case, dtype), distance=combo[1], scale=combo[2], alpha=combo[3], lambdas=combo[4],
                                   grad=True)


def check_torch_module(solver, golden, dtype):
    """ConsistencyLoss(opt)(depths, metadata) on GPU tensors of the reference's layout: the array path's values, and
    (3 loss).backward() leaves three times the array path's gradient (the same kernels: within the bars above)."""
    combo = cc.COMBOS[11]
    case = cc.make_case("batch")
    npdt = np.dtype(dtype)
    td = getattr(torch, dtype)
    B, H, W = case["P"], case["H"], case["W"]
    total, terms, g = run(solver, combo, npdt)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=td, device=dev)
    opt = types.SimpleNamespace(distance_type_static=combo[1], distance_scale=combo[2], distance_alpha=combo[3],
                                lambda_static_reprojection=combo[4][0], lambda_static_disparity=combo[4][1],
                                lambda_static_depth_ratio=combo[4][2], recon="i3d")
    warp = t(case["warp_norm"]).view(B, 2, 2, H, W)
    warp_before = warp.clone()
    meta = {"extrinsics": t(case["extrinsics"]).view(B, 2, 3, 4), "intrinsics": t(case["intrinsics"]).view(B, 2, 4), "warp": warp,
            "geometry_consistency": {"flows": (t(case["flow_ab"]), t(case["flow_ba"])),
                                     "masks": (t(case["weight_ab"]).view(B, 1, H, W), t(case["weight_ba"]).view(B, 1, H, W))}}
    module = ConsistencyLoss(opt)
    depths = t(case["depth"]).view(B, 2, H, W).requires_grad_(True)
    loss, batch = module(depths, meta)
    assert loss.dtype == td and loss.shape == () and loss.requires_grad
    assert set(batch) == set(cr.TERMS) and all(v.shape == (B,) and not v.requires_grad for v in batch.values())
    # the same kernels on the same inputs: the forward repeats bit for bit (rounded to the tensors' dtype)
    assert float(loss) == float(npdt.type(total))
    for name in cr.TERMS:
        assert np.array_equal(batch[name].cpu().numpy(), terms[name].astype(npdt))
    (3 * loss).backward()
    bar = 1e-9 if dtype == "float64" else 8 * max(float(golden[f"{cc.combo_key(combo)}/delta_grad"]), EPS32)
    got = depths.grad.cpu().numpy().reshape(g.shape).astype(np.float64)
    margins.below(f"cons torch gradient {dtype}", np.abs(got - 3.0 * g).max() / np.abs(3.0 * g).max(), bar)
    assert torch.equal(warp, warp_before)      # not scaled in place
    # a non-contiguous depths: the same values, the gradient lands in the caller's layout
    wide = torch.zeros(B, 2, H, 2 * W, dtype=td, device=dev)
    wide[..., ::2] = depths.detach()
    wide.requires_grad_(True)
    strided = wide[..., ::2]
    assert not strided.is_contiguous()
    loss2, _ = module(strided, meta)
    assert float(loss2) == float(loss)
    loss2.backward()
    got2 = wide.grad[..., ::2].cpu().numpy().reshape(g.shape).astype(np.float64)
    margins.below(f"cons torch strided gradient {dtype}", np.abs(got2 - g).max() / np.abs(g).max(), bar)
    assert not wide.grad[..., 1::2].any()
    # no gradient asked: values only
    with torch.no_grad():
        loss3, _ = module(depths.detach(), meta)
    assert float(loss3) == float(loss) and not loss3.requires_grad
    try:
        module(depths.detach().cpu(), meta)
    except ValueError as e:
        assert "GPU" in str(e)
    else:
        raise AssertionError("a CPU tensor was accepted")


def check_misaligned_tables(golden, dtype):
    """Tables that are not aligned to four elements take the one-pixel-per-thread kernels (case `batch`: 24 x 40, four workgroups
    per image where the aligned run has one): depths, and in a second run one flow tensor, as contiguous views offset by one
    element.  Total, terms and gradient against the fixture with the bars of test_gpu_consistency.py for this combination: f64
    1e-10 relative and the gradient 1e-9 x max |g|; f32 total and gradient 8 x the reference's own f32 delta (never below 2^-23;
    that test sets no f32 bar for the terms, so they are checked in f64)."""
    combo = cc.COMBOS[11]
    key, case = cc.combo_key(combo), cc.make_case("batch")
    td = getattr(torch, dtype)
    B, H, W = case["P"], case["H"], case["W"]
    assert W % 4 == 0
    dev = torch.device("cuda", 0)
    ref_total, ref_terms, ref_g = float(golden[f"{key}/total"]), golden[f"{key}/terms"], golden[f"{key}/grad"]
    d_total, d_grad = float(golden[f"{key}/delta_total"]), float(golden[f"{key}/delta_grad"])
    opt = types.SimpleNamespace(distance_type_static=combo[1], distance_scale=combo[2], distance_alpha=combo[3],
                                lambda_static_reprojection=combo[4][0], lambda_static_disparity=combo[4][1],
                                lambda_static_depth_ratio=combo[4][2], recon="i3d")
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=td, device=dev)

    def shifted(a):
        flat = torch.zeros(a.size + 1, dtype=td, device=dev)
        flat[1:] = t(a).ravel()
        v = flat[1:].view(a.shape)
        assert v.is_contiguous() and v.data_ptr() % (4 * v.element_size()) != 0
        return v
    for which in ("depths", "flow"):
        depths = (shifted if which == "depths" else t)(case["depth"]).view(B, 2, H, W).detach().requires_grad_(True)
        assert (depths.data_ptr() % (4 * depths.element_size()) != 0) == (which == "depths")
        flow_ba = (shifted if which == "flow" else t)(case["flow_ba"])
        meta = {"extrinsics": t(case["extrinsics"]).view(B, 2, 3, 4), "intrinsics": t(case["intrinsics"]).view(B, 2, 4),
                "warp": t(case["warp_norm"]).view(B, 2, 2, H, W),
                "geometry_consistency": {"flows": (t(case["flow_ab"]), flow_ba),
                                         "masks": (t(case["weight_ab"]).view(B, 1, H, W), t(case["weight_ba"]).view(B, 1, H, W))}}
        loss, batch = ConsistencyLoss(opt)(depths, meta)
        loss.backward()
        g = depths.grad.cpu().numpy().reshape(ref_g.shape).astype(np.float64)
        what = f"cons misaligned {which} {dtype}"
        f64 = dtype == "float64"
        margins.below(f"{what} total", abs(float(loss) - ref_total) / abs(ref_total), 1e-10 if f64 else 8 * max(d_total, EPS32))
        margins.below(f"{what} grad", np.abs(g - ref_g).max() / np.abs(ref_g).max(), 1e-9 if f64 else 8 * max(d_grad, EPS32))
        if f64:
            tt = np.stack([batch[name].cpu().numpy() for name in cr.TERMS], 1)
            margins.below(f"{what} terms", np.max(np.abs(tt - ref_terms) / np.abs(ref_terms)), 1e-10)


if __name__ == "__main__":
    torch.cuda.init()
    s = api.Solver(0)
    check_torch_module(s, np.load(cr.GOLDEN), sys.argv[1])
    check_misaligned_tables(np.load(cr.GOLDEN), sys.argv[1])
    s.close()
    print("torch module ok")
