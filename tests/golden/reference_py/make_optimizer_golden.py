#!/usr/bin/env python3
"""Mint tests/golden/reference_py/optimizer_golden.npz: the REAL RAdam.step and ParameterLoss.__call__ of the reference
(optimizer/radam.py, loss/parameter_loss.py) and torch.optim.Adam of the installed torch, on CPU tensors, on the seeded table of
tests/optimizer_cases.py.

    python tests/golden/reference_py/make_optimizer_golden.py <reference checkout>

Recorded in float32 (the reference's RAdam computes in float32 whatever it is given) per configuration of optimizer_cases.CONFIGS,
at the elements optimizer_cases.sample_indices names: `<config>/p/<k>` after steps 1, 5, 6 and 8, `<config>/m` and `<config>/v`
after eight.  Per recorded array, over ALL elements of the tensors: `.../spread`, max |reference f32 - the float64 restatement of
tests/optimizer_reference.py|, the reference's own rounding spread and the yardstick of the f32 tests, and `.../scale`, the
array's largest magnitude (the spread is asserted to stay below 1e-5 of the scale: f32 rounding, nothing larger).  `loss/value` (float64 run), `loss/spread` (|float32 run - float64 run|), `loss/grad` at the sample
elements for d(GRAD_OUT loss).  `digest`: sha256 of the inputs; `sample`: the flat indices.

torch.optim.Adam also runs in float64 and must agree with the restatement to 1e-12 of each array's scale: the restatement is
then held to the reference at both precisions.  Only recorded results are written.
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import optimizer_cases as oc  # noqa: E402
from tests import optimizer_reference as orf  # noqa: E402


def reference_run(make, case, dtype):
    """p after every recorded step and the final moments of the optimizer make(params), flat like the case."""
    params = [torch.tensor(t.astype(dtype)).requires_grad_(True) for t in oc.tensors(case, case["p"])]
    opt = make(params)
    flat = lambda ts: np.concatenate([np.asarray(t.detach().numpy(), dtype).ravel() for t in ts])
    out = {}
    for k in range(1, oc.STEPS + 1):
        for p, g in zip(params, oc.tensors(case, case["g"][k - 1])):
            p.grad = torch.tensor(g.astype(dtype))
        opt.step()
        if k in oc.RECORDED_STEPS:
            out[f"p/{k}"] = flat(params)
    # (an empty tensor's state exists too: the reference creates it at its first step)
    out["m"] = flat([opt.state[p]["exp_avg"] for p in params])
    out["v"] = flat([opt.state[p]["exp_avg_sq"] for p in params])
    return out


def main(reference):
    sys.path.insert(0, reference)
    from loss.parameter_loss import ParameterLoss
    from optimizer.radam import RAdam
    warnings.simplefilter("ignore")      # (the reference's add_(Number, Tensor) overloads are deprecated, not removed)
    case = oc.make_case()
    used, sample = case["used"], oc.sample_indices(case)
    # positions of the flat elements in the concatenation of the tensors
    where = np.cumsum(used) - 1
    out = {"digest": np.frombuffer(oc.digest(case).encode(), np.uint8), "sample": sample}
    for config, (family, wd, sgd) in oc.CONFIGS.items():
        if family == "adam":
            make = lambda ps: torch.optim.Adam(ps, weight_decay=wd, foreach=False, **oc.HYPER)
        else:
            make = lambda ps: RAdam(ps, weight_decay=wd, degenerated_to_sgd=sgd, **oc.HYPER)
        ref32 = reference_run(make, case, np.float32)
        re64 = orf.run(config, case, np.float64)
        if family == "adam":
            ref64 = reference_run(make, case, np.float64)
            for k, a in ref64.items():
                err = np.abs(a - re64[k][used]).max() / np.abs(a).max()
                assert err < 1e-12, (config, k, err)
        for k, a in ref32.items():
            want = re64[k][used]
            assert np.isfinite(a).all()
            out[f"{config}/{k}"] = a[where[sample]].astype(np.float32)
            out[f"{config}/{k}/spread"] = np.float64(np.abs(a.astype(np.float64) - want).max())
            out[f"{config}/{k}/scale"] = np.float64(np.abs(want).max())
            # the spread is the f32 tests' yardstick: it must be rounding, not a restatement that computes something else
            assert out[f"{config}/{k}/spread"] < 1e-5 * out[f"{config}/{k}/scale"], (config, k)
            print(f"{config}/{k}: spread {out[f'{config}/{k}/spread']:.3e}  scale {out[f'{config}/{k}/scale']:.3e}  "
                  f"ratio {out[f'{config}/{k}/spread'] / out[f'{config}/{k}/scale']:.2e}")
    opt = types.SimpleNamespace(lambda_parameter=oc.LAMBDA)
    values = {}
    for dtype in (np.float32, np.float64):
        params = [torch.tensor(t.astype(dtype)).requires_grad_(True) for t in oc.tensors(case, case["p"])]
        inits = [torch.tensor(t.astype(dtype)) for t in oc.tensors(case, case["p0"])]
        value, batch = ParameterLoss(inits, opt)(p for p in params)
        assert batch["parameter_loss"].shape == (1, 1)
        (oc.GRAD_OUT * value).backward()
        values[dtype] = (float(value), np.concatenate([p.grad.numpy().ravel() for p in params]))
    out["loss/value"] = np.float64(values[np.float64][0])
    out["loss/spread"] = np.float64(abs(values[np.float32][0] - values[np.float64][0]))
    out["loss/grad"] = values[np.float32][1][where[sample]].astype(np.float32)
    for dtype in values:     # the subgradient is exact in either precision: (lambda grad_out) sign(p - p0), ties 0
        assert np.array_equal(values[dtype][1], orf.loss_grad(case, dtype)[used]), dtype
    assert abs(values[np.float64][0] - orf.loss(case, np.float64)) <= 1e-12 * abs(values[np.float64][0])
    print(f"loss {out['loss/value']:.12g}  spread {out['loss/spread'] / out['loss/value']:.2e} relative")
    np.savez_compressed(orf.GOLDEN, **out)
    size = os.path.getsize(orf.GOLDEN)
    print(f"{orf.GOLDEN}: {size} bytes, {sample.size} sample elements of {int(used.sum())}")
    assert size < 1 << 20


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
