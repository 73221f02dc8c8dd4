"""GPU checks of the backbone's training operators (robust_cvd_amd/csrc/cvd_resnext_grad.h) through the array paths
(Solver.resnext_norm_train, resnext_norm_grad, resnext_grouped_conv_grad_input / _grad_weight, resnext_conv_grad_input /
_grad_weight, resnext_maxpool_grad) and, in a fresh process, through robust_cvd_amd.midas_train (tests/resnext_grad_torch_child.py).

Bar per tensor: |kernel - f64| <= 8 x max(delta, 2^-23 x scale) against the float64 restatement (tests/resnext_grad_reference.py),
delta = stock torch's own f32 error against that restatement, scale = the largest |value|, both read from the fixture
(tests/golden/reference_py/resnext_grad_golden.npz, minted on the CPU from stock torch autograd; never from these kernels); against
the stored f32 values that bar + delta.  The planted cases and the pool are exact resp. hold to the same bar."""
import os
import subprocess
import sys

import numpy as np
import pytest

from robust_cvd_amd import api
from tests import margins
from tests import resnext_grad_cases as gc
from tests import resnext_grad_reference as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    return api.Solver(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(gr.GOLDEN)


def check(key, tensor, golden, got, want, exact=False):
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all(), (key, tensor)
    delta, scale = float(golden[f"{key}/{tensor}_delta"]), float(golden[f"{key}/{tensor}_scale"])
    bar = gr.bar(delta, scale)
    err = float(np.abs(got - want).max())
    print(f"{key}/{tensor}: max |kernel - f64| {err:.3e}, bar {bar:.3e}, share {err / bar if bar else 0.0:.3f} (stock torch's own delta {delta:.3e})")
    if exact:
        assert err == 0.0, (key, tensor, err)
        return
    margins.below(f"resnext grad {key}/{tensor}", err, bar)
    if f"{key}/{tensor}" in golden.files:
        margins.below(f"resnext grad {key}/{tensor} vs reference", float(np.abs(got - golden[f"{key}/{tensor}"]).max()), bar + delta)


def copies(case):
    return {k: v.copy() for k, v in case.items() if isinstance(v, np.ndarray)}


def unchanged(case, before):
    return all(np.array_equal(case[k], v) for k, v in before.items())


def run_norm(solver, case):
    fwd = solver.resnext_norm_train(case["c"], case["norm"], gc.EPS, gc.MOMENTUM, case["training"], case["relu"], case["residual"])
    return fwd


@pytest.mark.parametrize("name", gc.NORM_CASES)
def test_norm_forward_and_backward(solver, golden, name):
    case = gc.make_norm_case(name)
    before = copies(case)
    norm_before = [a.copy() for a in case["norm"]]
    (wy, wmean, winv, wrm, wrv), (wgc, wgg, wgb, wgr) = gr.norm_case(case)
    key = "norm/" + name
    y, mean, invstd, rmean, rvar = run_norm(solver, case)
    check(key, "y", golden, y, wy)
    check(key, "running_mean", golden, rmean, wrm)
    check(key, "running_var", golden, rvar, wrv)
    # the saved vectors are the f64 statistics rounded once
    assert np.abs(mean - wmean).max() <= 2.0 ** -23 * max(np.abs(wmean).max(), 1e-30)
    assert np.abs(invstd - winv).max() <= 2.0 ** -23 * np.abs(winv).max()
    if not case["training"]:
        assert np.array_equal(rmean, case["norm"][2]) and np.array_equal(rvar, case["norm"][3]) and np.array_equal(mean, case["norm"][2])
    if name == "constant_channel":
        assert mean[1] == np.float32(0.75) and invstd[1] == np.float32(1.0 / np.sqrt(gc.EPS))
    again = run_norm(solver, case)
    assert all(np.array_equal(a, b) for a, b in zip((y, mean, invstd, rmean, rvar), again)), "a repeat differs"
    # backward on the restatement's mask tensor and statistics, so both sides read one mask
    masked = case["relu"] or case["residual"] is not None
    ymask = wy.astype(np.float32) if masked else None
    args = (case["gy"], case["c"], wmean.astype(np.float32), winv.astype(np.float32), case["norm"][0])
    got = solver.resnext_norm_grad(*args, y=ymask, training=case["training"], residual=case["residual"] is not None)
    check(key, "gc", golden, got[0], wgc)
    check(key, "g_gamma", golden, got[1], wgg)
    check(key, "g_beta", golden, got[2], wgb)
    if case["residual"] is not None:
        assert np.array_equal(got[3], np.where(ymask > 0, case["gy"], np.float32(0)))
    else:
        assert got[3] is None
    rep = solver.resnext_norm_grad(*args, y=ymask, training=case["training"], residual=case["residual"] is not None)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], rep[:3])), "a repeat differs"
    assert unchanged(case, before) and all(np.array_equal(a, b) for a, b in zip(case["norm"], norm_before))


def test_norm_refusals(solver):
    case = gc.make_norm_case("plain_2x5x3x7")
    one = case["c"][:1, :, :1, :1]
    with pytest.raises(ValueError, match="more than 1 value"):
        solver.resnext_norm_train(one, case["norm"])
    with pytest.raises(ValueError, match="momentum None"):
        solver.resnext_norm_train(case["c"], case["norm"], momentum=None)
    # the library's own refusals, below the Python checks
    h = solver
    null = h._fn("resnext_norm_train_device")(h._h, 1, 5, 1, 1, None, None, None, None, None, api.C.c_double(1e-5), api.C.c_double(0.1),
                                              1, 0, None, None, None, None, None)
    assert null != 0 and "more than 1 value" in h._fn("last_error", api.C.c_char_p)(h._h).decode()
    null = h._fn("resnext_norm_train_device")(h._h, 2, 5, 3, 7, None, None, None, None, None, api.C.c_double(1e-5), api.C.c_double(0.1),
                                              1, 0, None, None, None, None, None)
    assert null != 0 and "null array" in h._fn("last_error", api.C.c_char_p)(h._h).decode()
    bad = h._fn("resnext_grouped_conv_grad_input_device")(h._h, 1, 5, 7, 4, 12, 1, None, None, None, None)
    assert bad != 0 and "12" in h._fn("last_error", api.C.c_char_p)(h._h).decode()
    bad = h._fn("resnext_conv_grad_input_device")(h._h, 1, 9, 11, 3, 64, 7, 2, None, None, None, None, None)
    assert bad != 0 and "kernel_size must be 1" in h._fn("last_error", api.C.c_char_p)(h._h).decode()


@pytest.mark.parametrize("name", gc.GROUPED_CASES)
def test_grouped_conv_gradients(solver, golden, name):
    case = gc.make_grouped_case(name)
    before = copies(case)
    wgx, wgw = gr.grouped_case(case)
    key, exact = "grouped/" + name, name.startswith("planted")
    cg = case["weight"].shape[1]
    gx = solver.resnext_grouped_conv_grad_input(case["gy"], case["weight"], case["x"].shape[2:], case["stride"])
    gw = solver.resnext_grouped_conv_grad_weight(case["gy"], case["x"], cg, case["stride"], split=case["split"])
    check(key, "gx", golden, gx, wgx, exact)
    check(key, "gw", golden, gw, wgw, exact)
    assert np.array_equal(gx, solver.resnext_grouped_conv_grad_input(case["gy"], case["weight"], case["x"].shape[2:], case["stride"]))
    assert np.array_equal(gw, solver.resnext_grouped_conv_grad_weight(case["gy"], case["x"], cg, case["stride"], split=case["split"]))
    if case["split"]:
        # every slice count sums the same f64 products: the rounded results agree to the last bit or one
        one = solver.resnext_grouped_conv_grad_weight(case["gy"], case["x"], cg, case["stride"], split=1)
        assert np.abs(one - gw).max() <= 2.0 ** -23 * np.abs(wgw).max()
    if exact:
        # <gy, conv(u)> = <dgrad(gy), u> = <wgrad(gy, u), W> on the kernels' own results
        y = gr.conv_forward(case["x"], case["weight"], case["stride"], case["groups"])
        a = float((case["gy"].astype(np.float64) * y).sum())
        assert a == float((gx.astype(np.float64) * case["x"]).sum()) == float((gw.astype(np.float64) * case["weight"]).sum())
    assert unchanged(case, before)


@pytest.mark.parametrize("name", gc.DENSE_CASES)
def test_dense_conv_gradients(solver, golden, name):
    case = gc.make_dense_case(name)
    before = copies(case)
    wgx, wgw = gr.dense_case(case)
    key, exact = "dense/" + name, name.startswith("planted")
    k = case["weight"].shape[2]
    gw = solver.resnext_conv_grad_weight(case["gy"], case["x"], k, case["stride"])
    check(key, "gw", golden, gw, wgw, exact)
    assert np.array_equal(gw, solver.resnext_conv_grad_weight(case["gy"], case["x"], k, case["stride"]))
    if k == 1:
        gx = solver.resnext_conv_grad_input(case["gy"], case["weight"], case["x"].shape[2:], case["stride"], add=case["add"])
        check(key, "gx", golden, gx, wgx, exact)
        assert np.array_equal(gx, solver.resnext_conv_grad_input(case["gy"], case["weight"], case["x"].shape[2:], case["stride"],
                                                                 add=case["add"]))
        if case["stride"] == 2:
            odd = np.ones(gx.shape[2:], bool)
            odd[::2, ::2] = False
            rest = np.zeros_like(gx) if case["add"] is None else case["add"]
            assert np.array_equal(gx[:, :, odd], rest[:, :, odd]), "the odd positions hold more than the addend"
    else:
        with pytest.raises(ValueError, match="kernel_size must be 1"):
            solver.resnext_conv_grad_input(case["gy"], case["weight"], case["x"].shape[2:], case["stride"])
    if exact:
        y = gr.conv_forward(case["x"], case["weight"], case["stride"], 1)
        a = float((case["gy"].astype(np.float64) * y).sum())
        assert a == float((gw.astype(np.float64) * case["weight"]).sum())
        if k == 1:
            assert a == float((gx.astype(np.float64) * case["x"]).sum())
    assert unchanged(case, before)


@pytest.mark.parametrize("name", gc.POOL_CASES)
def test_maxpool_gradient(solver, golden, name):
    case = gc.make_pool_case(name)
    before = copies(case)
    want = gr.maxpool_grad(case["x"], case["gy"])
    gx = solver.resnext_maxpool_grad(case["x"], case["gy"])
    check("pool/" + name, "gx", golden, gx, want)
    # where an element is the argmax of one window at most, the value is that window's gradient itself
    assert np.array_equal(gx != 0, want != 0)
    assert np.array_equal(gx, solver.resnext_maxpool_grad(case["x"], case["gy"]))
    assert unchanged(case, before)


def chained_block(solver, case):
    """The block through the operator calls, in the order the one-call pair runs them -> (saved table, running, gx, gw, gg, gb)."""
    x, ws, norms, stride, tr = case["x"], case["weights"], case["norms"], case["stride"], case["training"]
    down = len(ws) == 4
    norm = lambda c, i, relu=False, residual=None: solver.resnext_norm_train(c, norms[i], gc.EPS, gc.MOMENTUM, tr, relu, residual)
    c1 = solver.resnext_conv(x, ws[0])
    f1 = norm(c1, 0, True)
    c2 = solver.resnext_grouped_conv(f1[0], ws[1], stride=stride)
    f2 = norm(c2, 1, True)
    identity, cd, fd = x, None, None
    if down:
        cd = solver.resnext_conv(x, ws[3], stride=stride)
        fd = norm(cd, 3)
        identity = fd[0]
    c3 = solver.resnext_conv(f2[0], ws[2])
    f3 = norm(c3, 2, False, identity)
    saved, running = [], []
    for c, f in [(c1, f1), (c2, f2), (c3, f3)] + ([(cd, fd)] if down else []):
        saved += [c, f[1], f[2], f[0]]
        running.append([f[3], f[4]])
    grad = lambda g, c, f, i, mask=True, residual=False: solver.resnext_norm_grad(g, c, f[1], f[2], norms[i][0], y=f[0] if mask else None,
                                                                                  training=tr, residual=residual)
    gc3, gg3, gb3, gres = grad(case["gy"], c3, f3, 2, residual=True)
    gw3 = solver.resnext_conv_grad_weight(gc3, f2[0], 1, 1)
    g2 = solver.resnext_conv_grad_input(gc3, ws[2], f2[0].shape[2:], 1)
    gc2, gg2, gb2, _ = grad(g2, c2, f2, 1)
    gw2 = solver.resnext_grouped_conv_grad_weight(gc2, f1[0], ws[1].shape[1], stride)
    g1 = solver.resnext_grouped_conv_grad_input(gc2, ws[1], f1[0].shape[2:], stride)
    gc1, gg1, gb1, _ = grad(g1, c1, f1, 0)
    gw1 = solver.resnext_conv_grad_weight(gc1, x, 1, 1)
    gw, gg, gb, add = [gw1, gw2, gw3], [gg1, gg2, gg3], [gb1, gb2, gb3], gres
    if down:
        gcd, ggd, gbd, _ = grad(gres, cd, fd, 3, mask=False)
        gw.append(solver.resnext_conv_grad_weight(gcd, x, 1, stride))
        gg.append(ggd)
        gb.append(gbd)
        add = solver.resnext_conv_grad_input(gcd, ws[3], x.shape[2:], stride)
    gx = solver.resnext_conv_grad_input(gc1, ws[0], x.shape[2:], 1, add=add)
    return saved, running, gx, gw, gg, gb


@pytest.mark.parametrize("name", gc.BLOCK_CASES)
def test_block_call(solver, golden, name):
    """the three forms (downsample at stride 1 and at stride 2, identity) in training mode and one in eval mode: the one-call pair
    against the restatement and the fixture, and equal to the chained operator calls bit for bit (both routings of conv1's addend)"""
    case = gc.make_block_case(name)
    before = copies(case)
    want = gr.block_case(case)
    key = "block/" + name
    n = len(case["weights"])
    out, saved, running = solver.resnext_block_train(case["x"], case["weights"], case["norms"], case["stride"], gc.EPS, gc.MOMENTUM,
                                                     case["training"])
    assert [a.shape for a in saved] == api.resnext_block_saved_shapes(*case["x"].shape[:1], *case["x"].shape[2:], case["x"].shape[1],
                                                                      case["weights"][0].shape[0], case["weights"][2].shape[0],
                                                                      case["stride"], n == 4)
    assert out is saved[11]
    check(key, "out", golden, out, want["out"])
    for i in range(n):
        if case["training"]:
            check(key, f"rm{i}", golden, running[i][0], want[f"rm{i}"])
            check(key, f"rv{i}", golden, running[i][1], want[f"rv{i}"])
        else:
            assert np.array_equal(running[i][0], case["norms"][i][2]) and np.array_equal(running[i][1], case["norms"][i][3])
    gammas = [four[0] for four in case["norms"]]
    gx, gw, gg, gb = solver.resnext_block_backward(case["gy"], case["x"], case["weights"], gammas, saved, case["stride"], case["training"])
    check(key, "gx", golden, gx, want["gx"])
    for i in range(n):
        check(key, f"gw{i}", golden, gw[i], want[f"gw{i}"])
        check(key, f"gg{i}", golden, gg[i], want[f"gg{i}"])
        check(key, f"gb{i}", golden, gb[i], want[f"gb{i}"])
    # bit for bit the chained operators'
    csaved, crunning, cgx, cgw, cgg, cgb = chained_block(solver, case)
    assert all(np.array_equal(a, b) for a, b in zip(saved, csaved)), "the saved table differs from the chained operators'"
    assert all(np.array_equal(a, b) for pair, cpair in zip(running, crunning) for a, b in zip(pair, cpair))
    assert np.array_equal(gx, cgx)
    assert all(np.array_equal(a, b) for mine, theirs in ((gw, cgw), (gg, cgg), (gb, cgb)) for a, b in zip(mine, theirs))
    # a repeat is bit for bit; without the input gradient the rest is unchanged
    again = solver.resnext_block_backward(case["gy"], case["x"], case["weights"], gammas, saved, case["stride"], case["training"],
                                          input_gradient=False)
    assert again[0] is None and all(np.array_equal(a, b) for mine, theirs in zip((gw, gg, gb), again[1:]) for a, b in zip(mine, theirs))
    assert unchanged(case, before)


def test_torch_layer_in_a_fresh_process():
    """robust_cvd_amd.midas_train.ResNeXt / MidasNet on the GPU: torch is imported first, so the checks run in a child."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    done = subprocess.run([sys.executable, "-m", "tests.resnext_grad_torch_child"], cwd=root, capture_output=True, text=True, timeout=600)
    print(done.stdout)
    assert done.returncode == 0 and "all checks passed" in done.stdout, done.stdout[-4000:] + done.stderr[-4000:]
