"""Child process of tests/test_gpu_optimizer.py::test_torch_surface (python -m tests.optimizer_torch_child): torch is imported first,
then the library.  robust_cvd_amd.optimizer.create("Adam" | "RAdam") over eight steps against the reference's recorded run,
a torch.optim.Adam checkpoint continued, robust_cvd_amd.parameter_loss.ParameterLoss against the array path and inside JointLoss,
the number of entry-point calls per step / loss / backward, and the error cases."""
import copy
import ctypes as C
import types

import numpy as np
import torch

from robust_cvd_amd import api, optimizer, parameter_loss
from robust_cvd_amd import torch_common as tc
from robust_cvd_amd.joint_loss import JointLoss
from tests import margins
from tests import optimizer_cases as oc
from tests import optimizer_reference as orf

DEV = torch.device("cuda", 0)
SQUARE = 6      # the tensor of 64 elements is an 8 x 8 matrix whose gradient arrives transposed (not contiguous)


class CallCounter:
    """wraps solver._fn: counts the look-ups of one entry point (every call looks its entry point up)"""

    def __init__(self, solver, name):
        self.count, self.name, self.fn = 0, name, solver._fn
        solver._fn = self

    def __call__(self, name, *args, **kw):
        self.count += name == self.name
        return self.fn(name, *args, **kw)

    def close(self, solver):
        solver._fn = self.fn


def device_tensors(case, flat, dtype):
    out = [torch.tensor(t, dtype=dtype, device=DEV) for t in oc.tensors(case, flat)]
    out[SQUARE] = out[SQUARE].view(8, 8)
    return out


def flat_of(case, tensors, dtype):
    a = np.zeros(case["total"], dtype)
    for dst, t in zip(oc.tensors(case, a), tensors):
        dst[:] = t.detach().cpu().numpy().ravel()
    return a


def set_gradients(case, params, k, dtype, transpose=True):
    """fresh gradient tensors of step k (new addresses every step); the square one transposed in memory (transpose=False: not,
    for torch's fused Adam, which refuses a gradient whose layout is not its parameter's)"""
    for i, (p, g) in enumerate(zip(params, device_tensors(case, case["g"][k - 1], dtype))):
        if i == SQUARE and transpose:
            g = g.t().contiguous().t()
            assert not g.is_contiguous()
        p.grad = g


def check_create(golden, config):
    """Two param groups that carry the hyperparameters themselves (the defaults are wrong on purpose), a parameter that never gets
    a gradient in the middle of the list, gradients dropped with set_to_none between steps, one non-contiguous gradient: the
    recorded elements within the f32 bar, one entry-point call per step."""
    case = oc.make_case()
    family, wd, sgd = oc.CONFIGS[config]
    params = [p.requires_grad_(True) for p in device_tensors(case, case["p"], torch.float32)]
    frozen = torch.full((5,), 3.0, device=DEV, requires_grad=True)
    half = len(params) // 2
    hyper = dict(oc.HYPER, weight_decay=wd)
    groups = [dict(params=params[:half] + [frozen], **hyper), dict(params=params[half:], **hyper)]
    extra = {} if family == "adam" else dict(degenerated_to_sgd=sgd)
    opt = optimizer.create("Adam" if family == "adam" else "RAdam", groups, lr=0.5, betas=(0.5, 0.5), eps=1e-3, **extra)
    assert isinstance(opt, torch.optim.Optimizer) and isinstance(opt, optimizer.OPTIMIZER_MAP["Adam" if family == "adam" else "RAdam"])
    counter = CallCounter(tc.solver(DEV), "param_step_device")
    sample = golden["sample"]

    def compare(name, tensors):
        key = f"{config}/{name}"
        err = np.abs(flat_of(case, tensors, np.float32)[sample].astype(np.float64) - golden[key].astype(np.float64)).max()
        margins.below(f"opt torch {key}", err, orf.bar(golden, key))
    for k in range(1, oc.STEPS + 1):
        set_gradients(case, params, k, torch.float32)
        assert opt.step() is None
        opt.zero_grad(set_to_none=True)
        assert all(p.grad is None for p in params)
        if k in oc.RECORDED_STEPS:
            compare(f"p/{k}", params)
    assert counter.count == oc.STEPS, counter.count
    counter.close(tc.solver(DEV))
    compare("m", [opt.state[p]["exp_avg"] for p in params])
    compare("v", [opt.state[p]["exp_avg_sq"] for p in params])
    assert frozen not in opt.state and torch.all(frozen == 3.0)
    st = opt.state[params[1]]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and torch.is_tensor(st["step"]) and float(st["step"]) == oc.STEPS
    # a closure is evaluated with gradients enabled and its value returned; with no gradient anywhere nothing is launched
    assert opt.step(lambda: torch.ones(1, device=DEV, requires_grad=True).sum()).item() == 1.0
    # state_dict round trip into a fresh instance: the next step is the same
    twins = [p.detach().clone().requires_grad_(True) for p in params]
    groups = [dict(params=twins[:half] + [frozen.detach().clone().requires_grad_(True)], **hyper), dict(params=twins[half:], **hyper)]
    other = optimizer.create("Adam" if family == "adam" else "RAdam", groups, **extra)
    other.load_state_dict(copy.deepcopy(opt.state_dict()))     # (load_state_dict keeps tensors that need no conversion)
    set_gradients(case, params, 1, torch.float32)
    set_gradients(case, twins, 1, torch.float32)
    opt.step()
    other.step()
    assert all(torch.equal(a, b) for a, b in zip(params, twins))


def check_mixed_precisions_and_groups():
    """A float64 parameter beside float32 ones: one launch per precision; per-group lr and betas reach the kernel (against the
    restatement: a few roundings)."""
    a = torch.linspace(-1, 1, 37, device=DEV).requires_grad_(True)
    b = torch.linspace(-2, 2, 11, device=DEV, dtype=torch.float64).requires_grad_(True)
    opt = optimizer.Adam([dict(params=[a], lr=0.1, betas=(0.8, 0.9)), dict(params=[b], weight_decay=0.1)], lr=0.01)
    counter = CallCounter(tc.solver(DEV), "param_step_device")
    a0, b0 = a.detach().cpu().numpy().copy(), b.detach().cpu().numpy().copy()
    ga, gb = np.cos(np.arange(37)).astype(np.float32), np.sin(np.arange(11.0))
    a.grad, b.grad = torch.tensor(ga, device=DEV), torch.tensor(gb, device=DEV)
    opt.step()
    assert counter.count == 2, counter.count
    counter.close(tc.solver(DEV))
    wa = orf.apply_rule(api.adam_record(1, 0.1, (0.8, 0.9)), a0, ga, np.zeros_like(a0), np.zeros_like(a0))[0]
    wb = orf.apply_rule(api.adam_record(1, 0.01, weight_decay=0.1), b0, gb, np.zeros_like(b0), np.zeros_like(b0))[0]
    margins.below("opt groups f32", np.abs(a.detach().cpu().numpy() - wa).max(), 4 * orf.EPS32)
    margins.below("opt groups f64", np.abs(b.detach().cpu().numpy() - wb).max(), 2e-15)


def check_torch_checkpoint(golden, fused=False):
    """torch.optim.Adam runs three steps; its state_dict loads; both continue for three: the f32 bar of the recorded Adam run at
    step 6, on every element.  fused: torch's fused Adam, whose checkpoint keeps `step` on the GPU and says fused=True in its
    param groups: it loads, and `step` is on the CPU from the first step on (reading it never waits for the device)."""
    case = oc.make_case()
    config = "adam-wd0.01"
    hyper = dict(oc.HYPER, weight_decay=oc.CONFIGS[config][1])
    theirs = [p.requires_grad_(True) for p in device_tensors(case, case["p"], torch.float32)]
    ours = [p.detach().clone().requires_grad_(True) for p in theirs]
    ref = torch.optim.Adam(theirs, fused=fused, **hyper)
    for k in range(1, 4):
        set_gradients(case, theirs, k, torch.float32, transpose=not fused)
        ref.step()
    with torch.no_grad():
        for a, b in zip(ours, theirs):
            a.copy_(b)
    opt = optimizer.create("Adam", ours, **hyper)
    opt.load_state_dict(copy.deepcopy(ref.state_dict()))      # (a copy: loaded as they are, the moments would be shared)
    assert float(opt.state[ours[1]]["step"]) == 3.0
    for k in range(4, 7):
        set_gradients(case, theirs, k, torch.float32, transpose=not fused)
        set_gradients(case, ours, k, torch.float32)
        ref.step()
        opt.step()
    used = case["used"]
    diff = np.abs(flat_of(case, ours, np.float64) - flat_of(case, theirs, np.float64))[used].max()
    margins.below(f"opt torch checkpoint fused={fused}", diff, orf.bar(golden, f"{config}/p/6"))
    assert float(opt.state[ours[1]]["step"]) == 6.0 and all(opt.state[p]["step"].device.type == "cpu" for p in ours)
    if fused:
        assert ref.state[theirs[1]]["step"].is_cuda and opt.param_groups[0]["fused"]


def aligned_layout(case):
    counts = case["counts"]
    offsets = np.concatenate([[0], np.cumsum((counts + 3) // 4 * 4)[:-1]]).astype(np.int64)
    moved = dict(case, offsets=offsets, total=int(offsets[-1] + (counts[-1] + 3) // 4 * 4))
    for k in ("p", "p0"):
        moved[k] = np.zeros(moved["total"])
        for dst, src in zip(oc.tensors(moved, moved[k]), oc.tensors(case, case[k])):
            dst[:] = src
    return moved


def check_parameter_loss(dtype):
    """On a generator of parameters: the array path's value bit for bit (separately allocated tensors are all aligned, so the
    array path gets every tensor at an aligned offset: the same chunks take the same path and sum in the same order), the exact
    subgradient, one entry-point call forwards and one backwards."""
    case = oc.make_case()
    npdt = np.dtype(str(dtype).split(".")[1])
    params = [p.requires_grad_(True) for p in device_tensors(case, case["p"], dtype)]
    inits = device_tensors(case, case["p0"], dtype)
    assert all(p.numel() == 0 or p.data_ptr() % 16 == 0 for p in params + inits)
    criterion = parameter_loss.ParameterLoss((p for p in inits), types.SimpleNamespace(lambda_parameter=oc.LAMBDA))
    solver = tc.solver(DEV)
    counter = CallCounter(solver, "parameter_l1_device")
    loss, batch = criterion(p for p in params)
    assert counter.count == 1, counter.count
    assert loss.shape == () and loss.dtype == dtype and loss.requires_grad and batch["parameter_loss"].shape == (1, 1)
    (oc.GRAD_OUT * loss).backward()
    assert counter.count == 2, counter.count
    counter.close(solver)
    moved = aligned_layout(case)
    total = solver.parameter_l1(moved["p"].astype(npdt), moved["p0"].astype(npdt), moved["counts"], oc.LAMBDA, offsets=moved["offsets"])
    assert float(loss) == float(npdt.type(total)), (float(loss), total)
    want = orf.loss_grad(case, npdt)
    for p, w in zip(params, oc.tensors(case, want)):
        assert p.grad.shape == p.shape and np.array_equal(p.grad.cpu().numpy().ravel(), w)
    with torch.no_grad():
        quiet, _ = criterion(params)
    assert not quiet.requires_grad and float(quiet) == float(loss)


def check_joint_loss():
    """JointLoss with only the parameter term on, in float64: the fused term within 1e-10 relative of the default (torch) path's
    (torch sums in another order), the parameters' gradients equal."""
    case = oc.make_case()
    zero = dict.fromkeys(("lambda_static_disparity", "lambda_static_reprojection", "lambda_static_depth_ratio", "lambda_scene_flow_static",
                          "lambda_smooth_reprojection", "lambda_smooth_disparity", "lambda_smooth_depth_ratio", "lambda_disparity_smooth",
                          "lambda_contrast_loss"), 0.0)
    opt = types.SimpleNamespace(lambda_parameter=oc.LAMBDA, recon="colmap", **zero)
    inits = device_tensors(case, case["p0"], torch.float64)
    depths = torch.ones(1, 2, 4, 4, dtype=torch.float64, device=DEV)
    results = []
    for fused in (False, True):
        params = [p.requires_grad_(True) for p in device_tensors(case, case["p"], torch.float64)]
        criterion = JointLoss(opt, inits, fused_parameter_loss=fused)
        assert isinstance(criterion.parameter_loss, parameter_loss.ParameterLoss) == fused
        loss, batch, scene_flow = criterion(None, None, depths, {}, params)
        assert loss.shape == (1,) and loss.dtype == torch.float64 and scene_flow is None and set(batch) == {"parameter_loss"}
        loss.sum().backward()
        results.append((float(loss[0]), float(batch["parameter_loss"][0, 0]), [p.grad.clone() for p in params]))
    (la, ba, ga), (lb, bb, gb) = results
    margins.below("joint fused parameter_loss", abs(bb - ba) / abs(ba), 1e-10)
    margins.below("joint fused total", abs(lb - la) / abs(la), 1e-10)
    assert all(torch.equal(x, y) for x, y in zip(ga, gb))
    assert JointLoss(types.SimpleNamespace(**dict(vars(opt), lambda_parameter=0.0)), fused_parameter_loss=True) is not None


def raises(kind, match, fn):
    try:
        fn()
    except kind as e:
        assert match in str(e), (match, str(e))
    else:
        raise AssertionError(f"no {kind.__name__} ({match})")


def check_errors():
    p = torch.ones(6, 4, device=DEV, requires_grad=True)
    ok = [torch.ones(3, device=DEV), p]
    opt1 = types.SimpleNamespace(lambda_parameter=1.0)
    crit = parameter_loss.ParameterLoss([torch.zeros(3, device=DEV), torch.zeros(6, 4, device=DEV)], opt1)
    crit(ok)
    raises(ValueError, "parameters[1] is on cpu", lambda: crit([ok[0], p.detach().cpu()]))
    raises(TypeError, "parameters[1] must be float32 or float64", lambda: crit([ok[0], p.detach().half()]))
    raises(ValueError, "parameters[1] of shape (4, 6) is not contiguous",
           lambda: parameter_loss.ParameterLoss([torch.zeros(3, device=DEV), torch.zeros(4, 6, device=DEV)], opt1)([ok[0], p.detach().t()]))
    raises(TypeError, "parameters[0] is not a tensor", lambda: crit([1.0, p]))
    raises(ValueError, "1 parameters for 2", lambda: crit([p]))
    raises(ValueError, "parameters_init[0] does not have the shape", lambda: crit([torch.ones(4, device=DEV), p]))
    for kw in ("amsgrad", "maximize", "fused", "capturable", "foreach", "differentiable", "decoupled_weight_decay"):
        raises(ValueError, kw, lambda: optimizer.create("Adam", [p], lr=0.1, **{kw: True}))
    optimizer.create("Adam", [p], lr=0.1, amsgrad=False, fused=None)
    raises(TypeError, "nesterov", lambda: optimizer.create("Adam", [p], lr=0.1, nesterov=True))
    raises(TypeError, "amsgrad", lambda: optimizer.create("RAdam", [p], lr=0.1, amsgrad=True))
    raises(ValueError, "betas[1] must lie in [0, 1)", lambda: optimizer.create("RAdam", [p], betas=(0.9, 1.0)))
    raises(ValueError, "lr must be >= 0", lambda: optimizer.create("Adam", [p], lr=-1.0))
    raises(KeyError, "AdamW", lambda: optimizer.create("AdamW", [p]))
    assert list(optimizer.OPTIMIZER_NAMES) == ["Adam", "RAdam"]
    for name in optimizer.OPTIMIZER_NAMES:
        opt = optimizer.create(name, [p], lr=0.1)
        keep = p.detach().clone()
        p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]], device=DEV), torch.ones(1, device=DEV), (6, 4))
        raises(RuntimeError, "does not support sparse gradients", opt.step)
        p.grad = None
        h = torch.ones(6, 4, device=DEV, dtype=torch.float16, requires_grad=True)
        h.grad = torch.ones_like(h)
        raises(TypeError, "parameters[0] must be float32 or float64", optimizer.create(name, [h], lr=0.1).step)
        c = torch.ones(3, requires_grad=True)
        c.grad = torch.ones(3)
        raises(ValueError, "parameters[0] is on cpu", optimizer.create(name, [c], lr=0.1).step)
        t = torch.ones(4, 6, device=DEV).t().requires_grad_(True)
        t.grad = torch.ones(6, 4, device=DEV)
        raises(ValueError, "parameters[0] of shape (6, 4) is not contiguous", optimizer.create(name, [t], lr=0.1).step)
        assert torch.equal(p.detach(), keep)
    # a checkpoint that asks for amsgrad is refused at the step
    opt = optimizer.create("Adam", [p], lr=0.1)
    opt.param_groups[0]["amsgrad"] = True
    p.grad = torch.ones_like(p)
    raises(ValueError, "amsgrad", opt.step)
    p.grad = None


def check_address_rejections():
    """The device entry points refuse a null and a misaligned address of a tensor with elements before any device work (the
    tensors keep their values); the address of an empty tensor may be null."""
    solver = tc.solver(DEV)
    for dtype, es in ((torch.float32, 4), (torch.float64, 8)):
        t = [torch.full((9,), 2.0, dtype=dtype, device=DEV) for _ in range(5)]
        total = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
        counts = (C.c_int64 * 2)(9, 0)
        desc = api.param_desc(dtype == torch.float64, 2)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rec = (api.ParamRecord * 2)(api.adam_record(1, 0.1), api.adam_record(1, 0.1))
        arr = lambda a: (C.c_void_p * 2)(a, None)
        good = [arr(x.data_ptr()) for x in t]

        def l1(p, p0, g):
            return solver._fn("parameter_l1_device")(solver._h, C.byref(desc), p, p0, counts, C.c_double(1.0), C.c_void_p(total.data_ptr()),
                                                     g, C.c_void_p(t[4].data_ptr()), C.c_int32(0), stream)

        def step(p, g, m, v):
            return solver._fn("param_step_device")(solver._h, C.byref(desc), p, g, m, v, counts, rec, stream)
        err = lambda: solver._lib.cvd_last_error(solver._h).decode()
        for k, name in enumerate(("p", "p0", "grad")):
            for bad, what in ((arr(None), f"{name}[0] is a null pointer"), (arr(t[k].data_ptr() + es // 2), f"{name}[0] = ")):
                a = good[:3]
                a[k] = bad
                assert l1(*a) != 0 and what in err(), (what, err())
                assert "misaligned" in err() or "null" in err()
        assert l1(None, good[1], None) != 0 and "null p" in err()
        assert solver._fn("parameter_l1_device")(solver._h, C.byref(desc), good[0], good[1], counts, C.c_double(1.0), None, None, None,
                                                 C.c_int32(0), stream) != 0 and "neither total nor grad" in err()
        assert l1(good[0], good[1], good[2]) == 0
        for k, name in enumerate(("p", "g", "m", "v")):
            for bad, what in ((arr(None), f"{name}[0] is a null pointer"), (arr(t[k].data_ptr() + es // 2), "misaligned")):
                a = good[:4]
                a[k] = bad
                assert step(*a) != 0 and what in err(), (what, err())
        torch.cuda.synchronize()
        assert float(total) == 0.0 and all(torch.all(x == 2.0) for x in t[:2] + t[3:]) and not t[2].any()


if __name__ == "__main__":
    torch.cuda.init()
    golden = np.load(orf.GOLDEN)
    assert bytes(golden["digest"]).decode() == oc.digest(oc.make_case())
    for config in oc.CONFIGS:
        check_create(golden, config)
    check_mixed_precisions_and_groups()
    check_torch_checkpoint(golden)
    check_torch_checkpoint(golden, fused=True)
    for dtype in (torch.float32, torch.float64):
        check_parameter_loss(dtype)
    check_joint_loss()
    check_errors()
    check_address_rejections()
    torch.cuda.synchronize()
    print("torch optimizer ok")
