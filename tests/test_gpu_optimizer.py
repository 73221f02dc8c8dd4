"""The parameter regulariser and the optimizer step on the GPU (robust_cvd_amd/csrc/cvd_paramstep.h) through the
host-array entry points (Solver.parameter_l1, Solver.param_step): the f64 kernels against the f64 restatement
(tests/optimizer_reference.py), the f32 kernels against the reference's recorded run
(tests/golden/reference_py/optimizer_golden.npz), the exact subgradient in both modes, bit-for-bit repeatability, the scalar
against the 16-byte path, tables of nothing and of one element, the rejections, and the torch surface (ParameterLoss, JointLoss's
fused_parameter_loss, optimizer.create) in a child process (tests/optimizer_torch_child.py).  Nothing here reads the reference
tree."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from robust_cvd_amd import api
from tests import margins
from tests import optimizer_cases as oc
from tests import optimizer_reference as orf

pytestmark = pytest.mark.gpu
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])


@pytest.fixture(scope="module")
def solver():
    s = api.Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def golden():
    g = np.load(orf.GOLDEN)
    assert bytes(g["digest"]).decode() == oc.digest(oc.make_case())
    return g


def gpu_run(solver, config, dtype, case=None, offsets=None, steps=oc.STEPS):
    """orf.run's dict from the kernels: `steps` calls of param_step over the case's layout (or over `offsets`)."""
    case = case or oc.make_case()
    offsets = case["offsets"] if offsets is None else offsets
    p = case["p"].astype(dtype)
    m, v = np.zeros_like(p), np.zeros_like(p)
    out = {}
    for k in range(1, steps + 1):
        p, m, v = solver.param_step(p, case["g"][k - 1].astype(dtype), m, v, case["counts"], orf.record(config, k), offsets=offsets)
        if k in oc.RECORDED_STEPS:
            out[f"p/{k}"] = p
    out["m"], out["v"] = m, v
    return out


@pytest.fixture(scope="module")
def f32_runs(solver):
    """The f32 kernels' eight steps of every configuration, computed once."""
    return {config: gpu_run(solver, config, np.float32) for config in oc.CONFIGS}


@pytest.mark.parametrize("config", list(oc.CONFIGS))
def test_f64_step_against_the_restatement(solver, config):
    """State and parameters within 1e-12 max |x| per array: a handful of roundings at 1.1e-16 on either side.  The elements
    between the tensors stay as they are."""
    case = oc.make_case()
    got, want = gpu_run(solver, config, np.float64), orf.run(config, case, np.float64)
    used = case["used"]
    for k, a in got.items():
        assert a.dtype == np.float64
        margins.below(f"opt f64 {config}/{k}", np.abs(a - want[k])[used].max() / np.abs(want[k][used]).max(), 1e-12)
        assert np.all(a[~used] == (7.0 if k.startswith("p") else 0.0)), k


@pytest.mark.parametrize("config", list(oc.CONFIGS))
def test_f32_step_against_the_reference(f32_runs, golden, config):
    """The yardstick is the reference's own f32 run against the f64 restatement, from the fixture (never below one f32 rounding
    of the array's scale); the factor 8 covers operation order, contraction and the device's sqrt and division."""
    for k, a in f32_runs[config].items():
        key = f"{config}/{k}"
        assert a.dtype == np.float32
        err = np.abs(a[golden["sample"]].astype(np.float64) - golden[key].astype(np.float64)).max()
        margins.below(f"opt f32 {key}", err, orf.bar(golden, key), info=("reference f32 spread", float(golden[f"{key}/spread"])))


@pytest.mark.parametrize("config", list(oc.CONFIGS))
def test_f32_step_against_the_f32_restatement_everywhere(f32_runs, golden, config):
    """The fixture holds sample elements; every other element is held to the f32 restatement (itself within the bar of the
    fixture: tests/test_optimizer_reference.py) at the same bar."""
    case = oc.make_case()
    want, used = orf.run(config, case, np.float32), case["used"]
    for k, a in f32_runs[config].items():
        err = np.abs(a.astype(np.float64) - want[k].astype(np.float64))[used].max()
        margins.below(f"opt f32 all {config}/{k}", err, orf.bar(golden, f"{config}/{k}"))


def test_loss_against_the_restatement_and_the_reference(solver, golden):
    case = oc.make_case()
    value = float(golden["loss/value"])
    layout = dict(counts=case["counts"], offsets=case["offsets"])
    got64 = solver.parameter_l1(case["p"], case["p0"], lam=oc.LAMBDA, **layout)
    margins.below("opt loss f64", abs(got64 - orf.loss(case, np.float64)) / value, 1e-12)
    margins.below("opt loss f64 reference", abs(got64 - value) / value, 1e-12)
    got32 = solver.parameter_l1(case["p"].astype(np.float32), case["p0"].astype(np.float32), lam=oc.LAMBDA, **layout)
    margins.below("opt loss f32", abs(got32 - value), 8 * max(float(golden["loss/spread"]), orf.EPS32 * value),
                  info=("reference f32 spread", float(golden["loss/spread"])))


@DTYPES
def test_loss_gradient_is_exact_in_both_modes(solver, golden, dtype):
    """lambda sign(p - p0) grad_out with ties at zero, exactly; accumulate adds it to a prefilled table (one addition in the
    tensors' precision); the elements between the tensors are not written."""
    case = oc.make_case()
    used = case["used"]
    args = (case["p"].astype(dtype), case["p0"].astype(dtype))
    kw = dict(counts=case["counts"], offsets=case["offsets"], lam=oc.LAMBDA, grad_out=oc.GRAD_OUT)
    want = orf.loss_grad(case, dtype)
    total, g = solver.parameter_l1(*args, grad=True, **kw)
    assert g.dtype == dtype and np.array_equal(g, want)
    ties = (case["p"] == case["p0"]) & used
    assert ties.sum() > used.sum() // 4 and not g[ties].any()
    if dtype == np.float32:
        assert np.array_equal(g[golden["sample"]], golden["loss/grad"])
    assert total == solver.parameter_l1(*args, **{k: v for k, v in kw.items() if k != "grad_out"})
    pre = np.random.default_rng(5).normal(0.0, 1.0, case["total"]).astype(dtype)
    keep = pre.copy()
    _total, acc = solver.parameter_l1(*args, grad=pre, **kw)
    assert np.array_equal(pre, keep) and np.array_equal(acc, np.where(used, pre + want, pre))


@DTYPES
def test_timing_returns_times_and_the_same_results(solver, dtype):
    """kernel_ms of the host entry points (HIP events around the launches): finite and positive for every phase that ran, 0 for
    the gradient's when none is asked for, and the results are those of the untimed call."""
    case = oc.make_case()
    args = (case["p"].astype(dtype), case["p0"].astype(dtype))
    kw = dict(counts=case["counts"], offsets=case["offsets"], lam=oc.LAMBDA)
    plain = solver.parameter_l1(*args, **kw)
    total, ms = solver.parameter_l1(*args, timing=True, **kw)
    assert total == plain and np.isfinite(ms["forward"]) and 0.0 < ms["forward"] < 1e3 and ms["backward"] == 0.0
    _t, g = solver.parameter_l1(*args, grad=True, grad_out=oc.GRAD_OUT, **kw)
    total, g2, ms = solver.parameter_l1(*args, grad=True, grad_out=oc.GRAD_OUT, timing=True, **kw)
    assert total == plain and np.array_equal(g, g2)
    assert all(np.isfinite(ms[k]) and 0.0 < ms[k] < 1e3 for k in ("forward", "backward")), ms
    step = (args[0], case["g"][0].astype(dtype), np.zeros_like(args[0]), np.zeros_like(args[0]), case["counts"], orf.record("adam-wd0.01", 1))
    a = solver.param_step(*step, offsets=case["offsets"])
    b = solver.param_step(*step, offsets=case["offsets"], timing=True)
    assert len(b) == 4 and np.isfinite(b[3]) and 0.0 < b[3] < 1e3 and all(np.array_equal(x, y) for x, y in zip(a, b[:3]))


@DTYPES
def test_results_repeat_bit_for_bit(solver, dtype):
    case = oc.make_case()
    layout = dict(counts=case["counts"], offsets=case["offsets"])
    a = solver.parameter_l1(case["p"].astype(dtype), case["p0"].astype(dtype), lam=oc.LAMBDA, **layout)
    b = solver.parameter_l1(case["p"].astype(dtype), case["p0"].astype(dtype), lam=oc.LAMBDA, **layout)
    assert a == b and a > 0
    for config in ("adam-wd0.01", "radam-wd0.01-sgd"):
        x, y = gpu_run(solver, config, dtype, steps=6), gpu_run(solver, config, dtype, steps=6)
        assert all(np.array_equal(x[k], y[k]) for k in x), config


@DTYPES
def test_misaligned_view_matches_an_aligned_copy(solver, dtype):
    """MISALIGNED starts one element off a 16-byte boundary and goes element by element; the same data laid out with every
    tensor aligned goes 16 bytes per lane.  Same per-element function, no contraction: the same bits in every element."""
    case = oc.make_case()
    counts = case["counts"]
    aligned = np.concatenate([[0], np.cumsum((counts + 3) // 4 * 4)[:-1]]).astype(np.int64)
    assert case["offsets"][oc.MISALIGNED] % 4 == 1 and not (aligned % 4).any()
    moved = dict(case, offsets=aligned, total=int(aligned[-1] + (counts[-1] + 3) // 4 * 4))
    for k in ("p", "p0"):
        moved[k] = np.full(moved["total"], 7.0)
        for dst, src in zip(oc.tensors(moved, moved[k]), oc.tensors(case, case[k])):
            dst[:] = src
    moved["g"] = np.full((oc.STEPS, moved["total"]), 0.5)
    for s in range(oc.STEPS):
        for dst, src in zip(oc.tensors(moved, moved["g"][s]), oc.tensors(case, case["g"][s])):
            dst[:] = src
    t = oc.MISALIGNED
    for config in ("adam-wd0.01", "radam-wd0.01-sgd"):      # (six steps: both RAdam regimes)
        x, y = gpu_run(solver, config, dtype, steps=6), gpu_run(solver, config, dtype, case=moved, steps=6)
        for k in x:
            assert np.array_equal(oc.tensors(case, x[k])[t], oc.tensors(moved, y[k])[t]), (config, k)
            assert all(np.array_equal(a, b) for a, b in zip(oc.tensors(case, x[k]), oc.tensors(moved, y[k]))), (config, k)
    kw = dict(counts=counts, lam=oc.LAMBDA, grad_out=oc.GRAD_OUT, grad=True)
    _ta, ga = solver.parameter_l1(case["p"].astype(dtype), case["p0"].astype(dtype), offsets=case["offsets"], **kw)
    _tb, gb = solver.parameter_l1(moved["p"].astype(dtype), moved["p0"].astype(dtype), offsets=aligned, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(oc.tensors(case, ga), oc.tensors(moved, gb)))


@DTYPES
def test_empty_tensors_and_a_table_of_one_element(solver, dtype):
    one = np.array([0.75], dtype)
    r = api.adam_record(1, 0.1)
    # no tensor at all, one empty tensor, an empty tensor beside one element
    assert solver.parameter_l1(one[:0], one[:0], [], lam=2.0) == 0.0
    total, g = solver.parameter_l1(one, one + 1, [0], lam=2.0, grad=True)
    assert total == 0.0 and not g.any()
    for counts, offsets in (([], None), ([0], None), ([0, 0], [0, 1])):
        p, m, v = solver.param_step(one, one, one, one, counts, [r] * len(counts), offsets=offsets)
        assert p[0] == one[0] and m[0] == one[0] and v[0] == one[0]
    total, g = solver.parameter_l1(one, one - dtype(0.5), [0, 1], lam=2.0, offsets=[0, 0], grad=True, grad_out=3.0)
    assert total == 1.0 and g[0] == 6.0
    zero = np.zeros(1, dtype)
    p, m, v = solver.param_step(one, np.array([0.5], dtype), zero, zero, [1, 0], [r, r], offsets=[0, 1])
    wp, wm, wv = orf.apply_rule(r, one, np.array([0.5], dtype), zero, zero)
    tol = 1e-15 if dtype == np.float64 else 4 * orf.EPS32
    assert abs(p[0] - wp[0]) <= tol and abs(m[0] - wm[0]) <= tol * 0.05 and abs(v[0] - wv[0]) <= tol * 0.0025
    assert p[0] < one[0] and m[0] > 0 and v[0] > 0


def test_rejections(solver):
    """Everything cvd_hip.h lists is refused with a message before any device work: the arrays keep their contents.  (A null or
    misaligned device address: tests/optimizer_torch_child.py, where there are device tensors to point at.)"""
    n = 8
    p = np.linspace(1.0, 2.0, n)
    g, m, v = np.full(n, 0.5), np.zeros(n), np.zeros(n)
    good = api.adam_record(1, 0.1)

    def step(counts=(5, 3), offsets=(0, 5), **fields):
        r = api.adam_record(1, 0.1)
        for k, val in fields.items():
            setattr(r, k, val)
        return solver.param_step(p, g, m, v, list(counts), [good, r], offsets=list(offsets))
    step()
    nan, inf = float("nan"), float("inf")
    bad = [("negative", lambda: step(counts=(5, -1))), ("leaves the flat arrays", lambda: step(offsets=(0, 6))),
           ("leaves the flat arrays", lambda: step(offsets=(-1, 5))),
           ("beta1 must be finite", lambda: step(beta1=nan)), ("beta2 must lie in", lambda: step(beta2=1.0)),
           ("beta1 must lie in", lambda: step(beta1=-0.1)), ("eps must be finite", lambda: step(eps=inf)),
           ("step must be finite", lambda: step(step=nan)), ("grad_decay must be finite", lambda: step(grad_decay=inf)),
           ("param_decay must be finite", lambda: step(param_decay=nan)), ("denom_scale must be finite", lambda: step(denom_scale=nan)),
           ("denom_scale must be > 0", lambda: step(denom_scale=0.0)),
           ("not a CVD_PARAM_RULE", lambda: step(rule=4)), ("not a CVD_PARAM_RULE", lambda: step(rule=-1)),
           ("lambda must be finite", lambda: solver.parameter_l1(p, g, [n], lam=nan)),
           ("lambda must be finite", lambda: solver.parameter_l1(p, g, [n], lam=inf)),
           ("negative", lambda: solver.parameter_l1(p, g, [-n], lam=1.0)),
           ("exceed the chunk list", lambda: solver.parameter_l1(p, g, [2 ** 63 - 1], lam=1.0)),
           ("exceed the chunk list", lambda: step(counts=(5, 2 ** 63 - 1))),
           ("leaves the flat arrays", lambda: solver.parameter_l1(p, g, [n + 1], lam=1.0)),
           ("grad_out must be finite", lambda: solver.parameter_l1(p, g, [n], lam=1.0, grad=True, grad_out=nan))]
    for what, fn in bad:
        with pytest.raises(RuntimeError, match=what):
            fn()
    with pytest.raises(TypeError, match="float32 or float64"):
        solver.parameter_l1(p.astype(np.int32), g.astype(np.int32), [n], lam=1.0)
    with pytest.raises(ValueError, match="records"):
        solver.param_step(p, g, m, v, [5, 3], [good])
    # the desc and null arrays, through the C entry points; the outputs keep their sentinels: nothing ran
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ip = lambda a: np.asarray(a, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    err = lambda: solver._lib.cvd_last_error(solver._h)
    total = C.c_double(-7.0)
    l1, st = solver._fn("parameter_l1"), solver._fn("param_step")
    off, cnt = np.array([0], np.int64), np.array([n], np.int64)
    tail = [C.c_double(1.0), C.byref(total), None, C.c_double(1.0), C.c_int32(0), None]
    desc = api.param_desc(1, 1)
    assert l1(solver._h, C.byref(desc), ip(off), ip(cnt), C.c_int64(n), vp(p), vp(g), *tail) == 0 and total.value != -7.0
    total.value = -7.0
    keep = p.copy()
    rec = (api.ParamRecord * 1)(good)
    descs = []
    for stale in (desc.struct_size - 8, C.sizeof(api.ParamDesc), C.sizeof(api.ParamDesc) | ((api.ABI_REVISION - 1) << 32)):
        d = api.param_desc(1, 1)
        d.struct_size = stale
        descs.append((d, b"struct_size"))
    descs += [(api.param_desc(2, 1), b"precision"), (api.param_desc(1, -1), b"num_tensors")]
    for d, what in descs:
        assert l1(solver._h, C.byref(d), ip(off), ip(cnt), C.c_int64(n), vp(p), vp(g), *tail) != 0 and what in err()
        assert st(solver._h, C.byref(d), ip(off), ip(cnt), C.c_int64(n), vp(p), vp(g), vp(m), vp(v), rec, None) != 0 and what in err()
    assert l1(solver._h, None, ip(off), ip(cnt), C.c_int64(n), vp(p), vp(g), *tail) != 0 and b"null desc" in err()
    for k, name in enumerate(("p", "p0")):
        a = [vp(p), vp(g)]
        a[k] = None
        assert l1(solver._h, C.byref(desc), ip(off), ip(cnt), C.c_int64(n), *a, *tail) != 0 and ("null " + name).encode() in err()
    t = list(tail)
    t[1] = None
    assert l1(solver._h, C.byref(desc), ip(off), ip(cnt), C.c_int64(n), vp(p), vp(g), *t) != 0 and b"null total" in err()
    assert l1(solver._h, C.byref(desc), None, ip(cnt), C.c_int64(n), vp(p), vp(g), *tail) != 0 and b"null offsets" in err()
    assert l1(solver._h, C.byref(desc), ip(off), None, C.c_int64(n), vp(p), vp(g), *tail) != 0 and b"null counts" in err()
    for k, name in enumerate(("p", "g", "m", "v")):
        a = [vp(p), vp(g), vp(m), vp(v)]
        a[k] = None
        assert st(solver._h, C.byref(desc), ip(off), ip(cnt), C.c_int64(n), *a, rec, None) != 0 and ("null " + name).encode() in err()
    assert st(solver._h, C.byref(desc), ip(off), ip(cnt), C.c_int64(n), vp(p), vp(g), vp(m), vp(v), None, None) != 0
    assert b"null records" in err()
    assert total.value == -7.0 and np.array_equal(p, keep) and not m.any() and not v.any()


def test_torch_surface():
    """optimizer.create, ParameterLoss and JointLoss(fused_parameter_loss=True) on GPU tensors, in a fresh process: torch has to
    be imported before libcvd_hip.so is loaded (the process then holds one HIP runtime, torch's).  The checks are
    tests/optimizer_torch_child.py's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.optimizer_torch_child"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch optimizer ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
