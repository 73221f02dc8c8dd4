"""Mints tests/golden/reference_py/resnext_grad_golden.npz on the CPU from STOCK TORCH f32 ops and autograd (nn.functional.batch_norm,
conv2d, max_pool2d) -- never from the kernels -- for the cases of tests/resnext_grad_cases.py.  Per case and tensor: torch's f32
result, its distance `delta` from the float64 restatement (tests/resnext_grad_reference.py) and the restatement's scale; per case the
digest of its inputs.  Run from the repository root:  python tests/golden/reference_py/make_resnext_grad_golden.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", "..")))
from tests import resnext_grad_cases as gc          # noqa: E402
from tests import resnext_grad_reference as gr      # noqa: E402

F = torch.nn.functional


def t(a, grad=False):
    return torch.from_numpy(np.array(a)).requires_grad_(grad)


def torch_norm(case):
    c, gamma, beta = t(case["c"], True), t(case["norm"][0], True), t(case["norm"][1], True)
    rmean, rvar = t(case["norm"][2]), t(case["norm"][3])
    residual = None if case["residual"] is None else t(case["residual"], True)
    y = F.batch_norm(c, rmean, rvar, gamma, beta, case["training"], gc.MOMENTUM, gc.EPS)
    if case["relu"]:
        y = F.relu(y)
    if residual is not None:
        y = F.relu(y + residual)
    y.backward(t(case["gy"]))
    out = {"y": y, "running_mean": rmean, "running_var": rvar, "gc": c.grad, "g_gamma": gamma.grad, "g_beta": beta.grad}
    if residual is not None:
        out["g_residual"] = residual.grad
    return {k: v.detach().numpy() for k, v in out.items()}


def torch_conv(case, groups):
    x, w = t(case["x"], True), t(case["weight"], True)
    F.conv2d(x, w, None, case["stride"], w.shape[2] // 2, 1, groups).backward(t(case["gy"]))
    gx = x.grad.numpy()
    return {"gx": gx if case.get("add") is None else gx + case["add"], "gw": w.grad.numpy()}


def torch_pool(case):
    x = t(case["x"], True)
    F.max_pool2d(x, 3, 2, 1).backward(t(case["gy"]))
    return {"gx": x.grad.numpy()}


def torch_block(case):
    """torchvision's Bottleneck.forward (v1.5) in stock ops, then autograd."""
    tr = case["training"]
    x = t(case["x"], True)
    ws = [t(w, True) for w in case["weights"]]
    ns = [[t(four[0], True), t(four[1], True), t(four[2]), t(four[3])] for four in case["norms"]]
    bn = lambda v, i: F.batch_norm(v, ns[i][2], ns[i][3], ns[i][0], ns[i][1], tr, gc.MOMENTUM, gc.EPS)
    y = F.relu(bn(F.conv2d(x, ws[0]), 0))
    y = F.relu(bn(F.conv2d(y, ws[1], None, case["stride"], 1, 1, case["groups"]), 1))
    y = bn(F.conv2d(y, ws[2]), 2)
    identity = x if len(ws) == 3 else bn(F.conv2d(x, ws[3], None, case["stride"]), 3)
    y = F.relu(y + identity)
    y.backward(t(case["gy"]))
    out = {"out": y.detach().numpy(), "gx": x.grad.numpy()}
    for i in range(len(ws)):
        out.update({f"gw{i}": ws[i].grad.numpy(), f"gg{i}": ns[i][0].grad.numpy(), f"gb{i}": ns[i][1].grad.numpy()})
        if tr:
            out.update({f"rm{i}": ns[i][2].numpy(), f"rv{i}": ns[i][3].numpy()})
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    out = {}

    def record(key, case, got, want):
        out[f"{key}/input_sha256"] = np.frombuffer(gc.input_digest(case).encode(), dtype=np.uint8)
        for name, ref in want.items():
            g = got[name]
            assert g.shape == ref.shape and g.dtype == np.float32, (key, name)
            if g.size <= gr.STORED_ELEMENTS:                     # (larger tensors: delta and scale only, the fixture stays small)
                out[f"{key}/{name}"] = g
            out[f"{key}/{name}_delta"] = np.float64(np.abs(g - ref).max())
            out[f"{key}/{name}_scale"] = np.float64(np.abs(ref).max())

    for name in gc.NORM_CASES:
        case = gc.make_norm_case(name)
        fwd, bwd = gr.norm_case(case)
        want = {"y": fwd[0], "running_mean": fwd[3], "running_var": fwd[4], "gc": bwd[0], "g_gamma": bwd[1], "g_beta": bwd[2]}
        if case["residual"] is not None:
            want["g_residual"] = bwd[3]
        record("norm/" + name, case, torch_norm(case), want)
    for name in gc.GROUPED_CASES:
        case = gc.make_grouped_case(name)
        gx, gw = gr.grouped_case(case)
        record("grouped/" + name, case, torch_conv(case, case["groups"]), {"gx": gx, "gw": gw})
    for name in gc.DENSE_CASES:
        case = gc.make_dense_case(name)
        gx, gw = gr.dense_case(case)
        record("dense/" + name, case, torch_conv(case, 1), {"gx": gx, "gw": gw})
    for name in gc.POOL_CASES:
        case = gc.make_pool_case(name)
        record("pool/" + name, case, torch_pool(case), {"gx": gr.maxpool_grad(case["x"], case["gy"])})
    for name in gc.BLOCK_CASES:
        case = gc.make_block_case(name)
        record("block/" + name, case, torch_block(case), gr.block_case(case))
    np.savez_compressed(gr.GOLDEN, **out)
    print(gr.GOLDEN, os.path.getsize(gr.GOLDEN), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
