"""numpy restatement of what robust_cvd_amd/csrc/cvd_paramstep.h computes, in a given dtype: the four update rules (torch.optim.Adam;
the reference's optimizer/radam.py: rectified, degenerated to SGD, moments only) and the parameter regulariser with its
subgradient (loss/parameter_loss.py).  Every array operation is one rounding in `dtype`, in the order of the Python it restates;
the step scalars are api.adam_record / api.radam_record's doubles, cast to `dtype` like the kernel casts them.  The loss is summed
in float64.  GOLDEN is the reference's own recorded run (tests/golden/reference_py/make_optimizer_golden.py)."""
import os

import numpy as np

from robust_cvd_amd import api
from tests import optimizer_cases as oc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "optimizer_golden.npz")
EPS32 = 2.0 ** -23
RULE = {v: k for k, v in api.PARAM_RULES.items()}


def record(config, step):
    """The ParamRecord of step number `step` of a configuration of optimizer_cases.CONFIGS."""
    family, wd, sgd = oc.CONFIGS[config]
    if family == "adam":
        return api.adam_record(step, weight_decay=wd, **oc.HYPER)
    return api.radam_record(step, weight_decay=wd, degenerated_to_sgd=sgd, **oc.HYPER)


def apply_rule(r, p, g, m, v):
    """One step of the rule record r names on arrays of one dtype: the new (p, m, v)."""
    dt = p.dtype.type
    rule = RULE[r.rule]
    beta1, beta2, omb1, omb2 = dt(r.beta1), dt(r.beta2), dt(1.0 - r.beta1), dt(1.0 - r.beta2)
    if rule == "adam" and r.grad_decay != 0:
        g = g + dt(r.grad_decay) * p
    m = beta1 * m + omb1 * g
    v = beta2 * v + (omb2 * g) * g
    if rule == "moments":
        return p, m, v
    if rule == "adam":
        return p - dt(r.step) * (m / (np.sqrt(v) / dt(r.denom_scale) + dt(r.eps))), m, v
    if r.param_decay != 0:
        p = p - dt(r.param_decay) * p
    if rule == "radam":
        return p - dt(r.step) * (m / (np.sqrt(v) + dt(r.eps))), m, v
    return p - dt(r.step) * m, m, v


def run(config, case, dtype, steps=oc.STEPS):
    """{"p/<k>": p after step k for the recorded steps, "m", "v": after the last}, flat arrays of `dtype` over the case's layout
    (elements between the tensors move too: they are elements like any other here)."""
    p = case["p"].astype(dtype)
    m, v = np.zeros_like(p), np.zeros_like(p)
    out = {}
    for k in range(1, steps + 1):
        p, m, v = apply_rule(record(config, k), p, case["g"][k - 1].astype(dtype), m, v)
        if k in oc.RECORDED_STEPS:
            out[f"p/{k}"] = p
    out["m"], out["v"] = m, v
    return out


def loss(case, dtype, lam=oc.LAMBDA):
    """lam sum |p - p0| over the tensors: differences and magnitudes in `dtype`, the sum in float64."""
    d = np.abs(case["p"].astype(dtype) - case["p0"].astype(dtype))[case["used"]]
    return lam * float(np.sum(d.astype(np.float64)))


def loss_grad(case, dtype, lam=oc.LAMBDA, grad_out=oc.GRAD_OUT):
    """(lam grad_out) sign(p - p0) in `dtype`, 0 between the tensors."""
    dt = np.dtype(dtype).type
    s = np.sign(case["p"].astype(dtype) - case["p0"].astype(dtype))
    return np.where(case["used"], (dt(lam) * dt(grad_out)) * s, dt(0)).astype(dtype)


def bar(golden, key):
    """The f32 bar of a recorded array: 8 x the reference's own f32-against-f64 spread, never below one f32 rounding of the
    array's largest magnitude (both from the fixture)."""
    return 8.0 * max(float(golden[f"{key}/spread"]), EPS32 * float(golden[f"{key}/scale"]))
