"""Drop-in for the reference's `optimizer` package (optimizer/__init__.py, optimizer/radam.py) on GPU tensors: `Adam` and `RAdam`
as torch.optim.Optimizer subclasses whose step() is ONE kernel launch over all parameters (csrc/cvd_paramstep.h),
instead of a Python loop of about ten elementwise launches per tensor (RAdam) or torch's multi-tensor kernels (Adam).

    import robust_cvd_amd.optimizer as optimizer
    opt = optimizer.create("RAdam", params, lr, betas=(0.9, 0.999))      # OPTIMIZER_MAP, OPTIMIZER_NAMES as in the reference
    loss.backward(); opt.step(); opt.zero_grad()

`Adam(params, lr, betas, eps, weight_decay)` computes what torch.optim.Adam of the installed torch computes with amsgrad=False,
maximize=False (coupled weight decay); `RAdam(params, lr, betas, eps, weight_decay, degenerated_to_sgd)` what the reference's class
computes: rectified from N_sma >= 5 on, below that plain momentum SGD (degenerated_to_sgd) or moments only, eps outside the bias
correction, the rectification folded into the step size.  The step scalars are formed here in double, as the Python they replace
forms them.  Per-parameter state: `step` (a CPU float32 tensor, as torch keeps it), `exp_avg`, `exp_avg_sq`: state_dict() and
load_state_dict() work, and a torch.optim.Adam checkpoint loads.  Param groups with their own lr, betas, eps and weight_decay, a
closure, parameters whose .grad is None (skipped) and non-contiguous gradients (read through a contiguous copy) are supported;
a sparse gradient raises RuntimeError as in the reference.  One step() is one launch per precision present (all parameters on
one GPU), enqueued on torch's current stream with no host synchronisation.

Differences from the reference: its RAdam always computes in float32, whatever the parameter's dtype; here float64 parameters keep
float64 state and arithmetic.  Its ten-slot `buffer` in the param groups, a cache of host scalars, is not reproduced.  Parameters
must be contiguous float32 / float64 GPU tensors: half precisions raise.  `amsgrad`, `maximize`, `foreach`, `fused`, `capturable`,
`differentiable` and `decoupled_weight_decay` raise ValueError when set in the constructor; in the param groups of a loaded
checkpoint the three that change the result (`amsgrad`, `maximize`, `decoupled_weight_decay`) raise at the step, and a `step`
tensor that torch's fused / capturable Adam kept on the GPU is moved to the CPU once.

Import this module (torch) before anything loads libcvd_hip.so, as robust_cvd_amd.consistency.
"""
import ctypes as C

import torch
from torch.optim.optimizer import Optimizer

from . import api
from . import torch_common as tc
from .parameter_loss import addresses, by_precision, check_parameters, element_counts

_UNSUPPORTED = ("amsgrad", "maximize", "foreach", "fused", "capturable", "differentiable", "decoupled_weight_decay")
# of these, what changes the RESULT: refused in a loaded checkpoint's param groups too (the others only pick one of torch's
# implementations of the same rule, and a checkpoint written by torch.optim.Adam(fused=True) loads)
_OTHER_RULES = ("amsgrad", "maximize", "decoupled_weight_decay")


def _check_hyper(who, lr, betas, eps, weight_decay):
    """The ranges the kernel's records accept (cvd_param_record): refused here, with the constructor's argument named."""
    for name, value in (("lr", lr), ("eps", eps), ("weight_decay", weight_decay)):
        if not value >= 0.0:
            raise ValueError(f"{who}: {name} must be >= 0 (got {value})")
    if len(betas) != 2:
        raise ValueError(f"{who}: betas must be a pair (got {betas!r})")
    for i, beta in enumerate(betas):
        if not 0.0 <= beta < 1.0:
            raise ValueError(f"{who}: betas[{i}] must lie in [0, 1) (got {beta})")


def _check_unsupported(who, options):
    for k, v in options.items():
        if k not in _UNSUPPORTED:
            raise TypeError(f"{who}: unexpected keyword argument {k!r}")
        if v:
            raise ValueError(f"{who}: {k}={v!r} is not supported (one fused HIP launch is the only implementation)")


class _TableOptimizer(Optimizer):
    """The step over the multi-tensor table; a subclass names the record of one (group, step)."""

    def _record(self, group, step):
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        who = type(self).__name__
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params, grads, records, steps = [], [], [], []
        for group in self.param_groups:
            _check_unsupported(who, {k: group[k] for k in _OTHER_RULES if k in group})
            cache = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse:
                    raise RuntimeError(f"{who} does not support sparse gradients")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                elif not torch.is_tensor(state["step"]):     # (a checkpoint of the reference's RAdam counts in a Python int)
                    state["step"] = torch.tensor(float(state["step"]), dtype=torch.float32)
                elif state["step"].device.type != "cpu":     # (torch's fused / capturable Adam keeps it on the GPU: moved once,
                    state["step"] = state["step"].detach().to("cpu", torch.float32)   # so that reading it never waits for the device)
                if g.dtype != p.dtype or g.device != p.device:
                    raise TypeError(f"{who}: the gradient of a {p.dtype} parameter on {p.device} is {g.dtype} on {g.device}")
                number = float(state["step"]) + 1
                if number not in cache:
                    cache[number] = self._record(group, number)
                params.append(p)
                grads.append(g if g.is_contiguous() else g.contiguous())
                records.append(cache[number])
                steps.append(state["step"])
        if not params:
            return loss
        exp_avg = [self.state[p]["exp_avg"] for p in params]
        exp_avg_sq = [self.state[p]["exp_avg_sq"] for p in params]
        check_parameters(who, params)
        check_parameters(who, exp_avg, "exp_avg")
        check_parameters(who, exp_avg_sq, "exp_avg_sq")
        for i, (p, m, v) in enumerate(zip(params, exp_avg, exp_avg_sq)):
            if m.dtype != p.dtype or v.dtype != p.dtype or m.shape != p.shape or v.shape != p.shape:
                raise ValueError(f"{who}: the state of parameters[{i}] ({tuple(p.shape)}, {p.dtype}) does not match it")
        device = params[0].device
        handle = tc.solver(device)
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for dt, idx in by_precision(params).items():
                pick = lambda a: [a[i] for i in idx]
                p = pick(params)
                rec = (api.ParamRecord * len(idx))(*pick(records))
                desc = api.param_desc(dt == torch.float64, len(idx))
                handle._check(handle._fn("param_step_device")(
                    handle._h, C.byref(desc), addresses(p), addresses(pick(grads)), addresses(pick(exp_avg)),
                    addresses(pick(exp_avg_sq)), element_counts(p), rec, stream))
        torch._foreach_add_(steps, 1)
        return loss


class Adam(_TableOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, **unsupported):
        if torch.is_tensor(lr):
            lr = float(lr)
        _check_hyper("Adam", lr, betas, eps, weight_decay)
        _check_unsupported("Adam", unsupported)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _record(self, group, step):
        return api.adam_record(step, float(group["lr"]), group["betas"], group["eps"], group["weight_decay"])


class RAdam(_TableOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, degenerated_to_sgd=True):
        _check_hyper("RAdam", lr, betas, eps, weight_decay)
        self.degenerated_to_sgd = degenerated_to_sgd
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _record(self, group, step):
        return api.radam_record(step, float(group["lr"]), group["betas"], group["eps"], group["weight_decay"],
                                self.degenerated_to_sgd)


# the reference's interface (optimizer.OPTIMIZER_MAP, OPTIMIZER_NAMES, create): the two names depth_fine_tuning.py offers
OPTIMIZER_MAP = dict(Adam=Adam, RAdam=RAdam)
OPTIMIZER_NAMES = tuple(OPTIMIZER_MAP)


def create(name, *args, **kwargs):
    """The optimizer called `name` (one of OPTIMIZER_NAMES) over the parameters and hyperparameters given."""
    if name not in OPTIMIZER_MAP:
        raise KeyError(f"unknown optimizer {name!r} (one of {', '.join(OPTIMIZER_NAMES)})")
    return OPTIMIZER_MAP[name](*args, **kwargs)
