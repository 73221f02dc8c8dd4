"""Child process of tests/test_gpu_spatial.py::test_torch_modules (python -m tests.spatial_torch_child <dtype>): torch is imported
first, then the library.  robust_cvd_amd.spatial_losses.DisparitySmoothLoss / ContrastLoss on GPU tensors against the array path
(Solver.spatial_losses) on the same inputs, the one-pixel against the four-pixel path through a view that is not aligned, and (in
float64) robust_cvd_amd.joint_loss.JointLoss against the reference's recorded JointLoss."""
import sys
import types

import numpy as np
import torch

from robust_cvd_amd import api, spatial_losses
from robust_cvd_amd.joint_loss import JointLoss
from robust_cvd_amd.spatial_losses import ContrastLoss, DisparitySmoothLoss, spatial_terms
from tests import margins
from tests import sceneflow_cases as sfc
from tests import spatial_cases as sc
from tests import spatial_reference as sr

DEV = torch.device("cuda", 0)


def options(combo):
    return types.SimpleNamespace(distance_type="l1", lambda_disparity_smooth=combo[1], sigma_color_grad=combo[2],
                                 lambda_contrast_loss=combo[3], lambda_contrast_thresh=combo[4])


def check_modules(solver, dtype, name):
    """The two modules return the array path's values bit for bit (the same kernels on the same inputs, no atomics), and
    (3 loss).backward() leaves exactly three times the array path's gradient."""
    case = sc.make_case(name)
    npdt, td = np.dtype(dtype), getattr(torch, dtype)
    B, N, H, W = case["B"], case["N"], case["H"], case["W"]
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=td, device=DEV)
    images, orig = t(case["image"]).view(B, N, 3, H, W), t(case["depth_orig"]).view(B, N, H, W)
    for setting in ("smooth", "contrast"):
        combo = (name,) + sc.SETTINGS[setting]
        total, smooth, _contrast, g = solver.spatial_losses(**sc.case_kwargs(case, npdt, combo), **sc.combo_kwargs(combo), grad=True)
        depths = t(case["depth"]).view(B, N, H, W).requires_grad_(True)
        if setting == "smooth":
            module = DisparitySmoothLoss(options(combo))
            loss, batch = module(images, depths)
            assert set(batch) == {"disparity_smooth"}
            b = batch["disparity_smooth"]
            assert b.shape == (B,) and b.dtype == td and not b.requires_grad
            assert np.array_equal(b.cpu().numpy(), smooth.astype(npdt))
            again = lambda d: module(images, d)[0]
        else:
            module = ContrastLoss(options(combo))
            loss = module(orig, depths)
            again = lambda d: module(orig, d)
        assert torch.is_tensor(loss) and loss.dtype == td and loss.shape == () and loss.requires_grad
        assert float(loss) == float(npdt.type(total))
        (3 * loss).backward()
        assert np.array_equal(depths.grad.cpu().numpy().reshape(g.shape), npdt.type(3) * g)
        with torch.no_grad():
            quiet = again(depths)
        assert not quiet.requires_grad and float(quiet) == float(loss)
        assert not again(depths.detach()).requires_grad
        # a view that is not contiguous: the last three columns of a wider table are not part of it
        wide = torch.zeros(B, N, H, W + 3, dtype=td, device=DEV)
        wide[..., :W] = depths.detach()
        wide[..., W:] = 1.0
        wide.requires_grad_(True)
        view = wide[..., :W]
        assert not view.is_contiguous()
        loss_v = again(view)
        assert float(loss_v) == float(loss)
        loss_v.backward()
        assert np.array_equal(wide.grad[..., :W].cpu().numpy().reshape(g.shape), g) and not wide.grad[..., W:].any()
        try:
            again(depths.detach().cpu())
        except ValueError as e:
            assert "GPU" in str(e)
        else:
            raise AssertionError("a CPU tensor was accepted")
    # both terms in one call: the array path's values
    combo = (name,) + sc.SETTINGS["both"]
    total, smooth, contrast, g = solver.spatial_losses(**sc.case_kwargs(case, npdt, combo), **sc.combo_kwargs(combo), grad=True)
    depths = t(case["depth"]).view(B, N, H, W).requires_grad_(True)
    lt, ls, lc = spatial_terms(depths, orig, images, lambda_disparity_smooth=combo[1], sigma_color_grad=combo[2],
                               lambda_contrast_loss=combo[3], contrast_thresh=combo[4])
    assert float(lt) == float(npdt.type(total)) and float(lc) == float(npdt.type(contrast))
    assert np.array_equal(ls.cpu().numpy(), smooth.astype(npdt)) and not ls.requires_grad and not lc.requires_grad
    lt.backward()
    assert np.array_equal(depths.grad.cpu().numpy().reshape(g.shape), g)


def check_vector_and_scalar_paths(dtype):
    """`aligned` once as it is (W = 40, aligned tensors: four pixels per thread) and once through views offset by one element,
    so that the alignment test fails (one pixel per thread).  The per-pixel arithmetic is the same text compiled without
    contraction: the gradients are bit-identical; the sums differ in their order: 1e-14 in f64 (values accumulate in f64 in
    both precisions)."""
    case = sc.make_case("aligned")
    td = getattr(torch, dtype)
    B, N, H, W = case["B"], case["N"], case["H"], case["W"]
    combo = ("aligned",) + sc.SETTINGS["both"]
    kw = dict(lambda_disparity_smooth=combo[1], sigma_color_grad=combo[2], lambda_contrast_loss=combo[3], contrast_thresh=combo[4])

    def shifted(a, shape):
        flat = torch.zeros(a.size + 1, dtype=td, device=DEV)
        flat[1:] = torch.tensor(np.ascontiguousarray(a).ravel(), dtype=td, device=DEV)
        v = flat[1:].view(shape)
        assert v.is_contiguous() and v.data_ptr() % (4 * v.element_size()) != 0
        return v
    t = lambda a, shape: torch.tensor(np.ascontiguousarray(a), dtype=td, device=DEV).view(shape)
    results = []
    for make in (t, shifted):
        depths = make(case["depth"], (B, N, H, W)).detach().requires_grad_(True)
        assert (depths.data_ptr() % (4 * depths.element_size()) == 0) == (make is t)
        total, smooth, contrast = spatial_terms(depths, make(case["depth_orig"], (B, N, H, W)), make(case["image"], (B, N, 3, H, W)),
                                                **kw)
        total.backward()
        results.append((float(total), smooth.double().cpu().numpy(), float(contrast), depths.grad.cpu().numpy()))
    a, b = results
    tol = 1e-14 if dtype == "float64" else 2.0 ** -23      # (f32: the f64 sums are rounded to f32 on return)
    margins.below(f"sp paths total {dtype}", abs(a[0] - b[0]) / abs(a[0]), tol)
    margins.below(f"sp paths smooth {dtype}", np.max(np.abs(a[1] - b[1]) / np.abs(a[1])), tol)
    margins.below(f"sp paths contrast {dtype}", abs(a[2] - b[2]) / abs(a[2]), tol)
    assert np.array_equal(a[3], b[3])


class CallCounter:
    """wraps solver._fn: counts the look-ups of one entry point (every call looks its entry point up)"""

    def __init__(self, solver, name):
        self.count, self.name, self.fn = 0, name, solver._fn
        solver._fn = self

    def __call__(self, name, *args, **kw):
        self.count += name == self.name
        return self.fn(name, *args, **kw)


def check_joint_loss(golden):
    """JointLoss in float64 against the reference's recorded JointLoss (recon = "colmap"): every entry of batch_losses within
    1e-10 relative, the depth gradient within 1e-9 x max |g|, the total within 8 x 2^-23 of the sum of the terms' magnitudes
    (the reference sums its total in a float32 tensor), the parameters' gradients lambda sign(p - p_init)."""
    case = sfc.make_case(sc.JOINT_CASE)
    assert bytes(golden["joint/digest"]).decode() == sfc.digest(case)
    extra = sc.joint_inputs(case)
    td = torch.float64
    B, H, W = case["P"], case["H"], case["W"]
    N = case["F"] // B
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=td, device=DEV)
    meta = {"extrinsics": t(case["extrinsics"]).view(B, N, 3, 4), "intrinsics": t(case["intrinsics"]).view(B, N, 4),
            "geometry_consistency": {"flows": tuple(t(f) for f in case["flows"]),
                                     "masks": tuple(t(m).view(B, 1, H, W) for m in case["masks"])},
            "temporal_smoothness": {"flows": tuple(t(f) for f in case["nflows"]),
                                    "masks": tuple(t(m).view(B, 1, H, W) for m in case["nmasks"]),
                                    "valid": t(case["valid"]).view(B, 2, 1)}}
    opt = types.SimpleNamespace(**sc.JOINT_OPTIONS)
    p_init = [t(p) for p in extra["parameters_init"]]
    params = [t(p).requires_grad_(True) for p in extra["parameters"]]
    criterion = JointLoss(opt, p_init)
    images, orig = t(extra["image"]).view(B, N, 3, H, W), t(extra["depth_orig"]).view(B, N, H, W)
    depths = t(case["depth"]).view(B, N, H, W).requires_grad_(True)
    counter = CallCounter(spatial_losses._solver(DEV), "spatial_losses_device")
    loss, batch, scene_flow = criterion(images, orig, depths, meta, params)
    assert counter.count == 1, counter.count      # both spatial terms: one kernel call
    assert loss.shape == (1,) and loss.dtype == td and loss.device == depths.device and scene_flow is None
    names = {k.split("/", 2)[2] for k in golden.files if k.startswith("joint/batch/")}
    assert set(batch) == names
    terms = [float(golden["joint/contrast"])]
    for k in sorted(names):
        ref = golden[f"joint/batch/{k}"]
        got = batch[k].detach().cpu().numpy()
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        margins.below(f"joint batch_losses {k}", np.max(np.abs(got - ref) / np.abs(ref)), 1e-10)
        terms.append(float(ref.sum()) if k == "parameter_loss" else float(ref.mean()))
    margins.below("joint total", abs(float(loss[0]) - float(golden["joint/total"])), 8 * 2.0 ** -23 * sum(abs(v) for v in terms))
    margins.below("joint total against its terms", abs(float(loss[0]) - sum(terms)) / sum(terms), 1e-10)
    loss.sum().backward()
    ref_g = golden["joint/grad"]
    # (the consistency and scene-flow gradients use float atomics on the product build: their own bar, 1e-9 x max |g|)
    margins.below("joint gradient", np.abs(depths.grad.cpu().numpy().reshape(ref_g.shape) - ref_g).max() / np.abs(ref_g).max(), 1e-9)
    lam = opt.lambda_parameter
    for i, (p, p0) in enumerate(zip(params, p_init)):
        want = lam * torch.sign(p.detach() - p0)
        assert torch.equal(p.grad, want) and np.array_equal(p.grad.cpu().numpy(), golden[f"joint/parameter_grad/{i}"])
    # one spatial term alone: still one call; neither: none
    for ls, lc, calls in ((0.0, 1.0, 1), (0.5, 0.0, 1), (0.0, 0.0, 0)):
        o = types.SimpleNamespace(**dict(sc.JOINT_OPTIONS, lambda_disparity_smooth=ls, lambda_contrast_loss=lc, lambda_parameter=0.0,
                                         lambda_scene_flow_static=0.0, lambda_smooth_reprojection=0.0, lambda_smooth_disparity=0.0,
                                         lambda_smooth_depth_ratio=0.0))
        counter.count = 0
        with torch.no_grad():
            l2, b2, _ = JointLoss(o)(images, orig, depths, meta)
        assert counter.count == calls and l2.shape == (1,) and ("disparity_smooth" in b2) == (ls > 0)
        assert {"reproj", "disp", "depth ratio"} <= set(b2)      # the consistency term on slices of the six-frame layout


if __name__ == "__main__":
    torch.cuda.init()
    dtype = sys.argv[1]
    s = api.Solver(0)
    for name in ("odd", "aligned", "six"):
        check_modules(s, dtype, name)
    check_vector_and_scalar_paths(dtype)
    if dtype == "float64":
        check_joint_loss(np.load(sr.GOLDEN))
    s.close()
    print("torch modules ok")
