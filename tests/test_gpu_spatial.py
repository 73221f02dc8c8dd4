"""Spatial smoothness and contrast losses on the GPU (robust_cvd_amd/csrc/cvd_spatial.h): the f64 and f32
kernels against the reference's committed outputs (tests/golden/reference_py/spatial_golden.npz), bit-for-bit repeatability of
values and gradient, the frame-wise structure, argument checks, and the torch modules and JointLoss over the device entry point
(tests/spatial_torch_child.py, which also compares the one- and the four-pixel path).  Nothing here reads the reference tree."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from robust_cvd_amd import api
from tests import margins
from tests import spatial_cases as sc
from tests import spatial_reference as sr

pytestmark = pytest.mark.gpu
IDS = [sc.combo_key(c) for c in sc.COMBOS]
EPS32 = 2.0 ** -23
ODD_BOTH = ("odd",) + sc.SETTINGS["both"]
ODD_CONTRAST = ("odd",) + sc.SETTINGS["contrast"]
ALIGNED_SECOND = ("aligned",) + sc.SETTINGS["second"]


@pytest.fixture(scope="module")
def solver():
    s = api.Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(sr.GOLDEN)


def run(solver, combo, dtype, grad=True, all_tables=False, **over):
    case = sc.make_case(combo[0])
    kw = dict(sc.case_kwargs(case, dtype, None if all_tables else combo), **sc.combo_kwargs(combo), grad=grad)
    kw.update(over)
    return solver.spatial_losses(**kw)


@pytest.mark.parametrize("combo", sc.COMBOS, ids=IDS)
def test_f64_kernel_against_the_reference(solver, golden, combo):
    """The project's bars for f64 against reference-held values: 1e-10 relative, the gradient 1e-9 x max |g|."""
    key, case = sc.combo_key(combo), sc.make_case(combo[0])
    assert bytes(golden[f"{combo[0]}/digest"]).decode() == sc.digest(case)
    total, smooth, contrast, g = run(solver, combo, np.float64)
    ref_total, ref_smooth, ref_contrast = float(golden[f"{key}/total"]), golden[f"{key}/smooth"], float(golden[f"{key}/contrast"])
    ref_g = golden[f"{key}/grad"]
    assert smooth.shape == (case["B"],) and g.shape == ref_g.shape and g.dtype == np.float64
    margins.below(f"sp f64 total {key}", abs(total - ref_total) / abs(ref_total), 1e-10)
    if combo[1] > 0:
        margins.below(f"sp f64 smooth {key}", np.max(np.abs(smooth - ref_smooth) / np.abs(ref_smooth)), 1e-10)
    else:
        assert not smooth.any() and not ref_smooth.any()
    if combo[3] > 0:
        margins.below(f"sp f64 contrast {key}", abs(contrast - ref_contrast) / abs(ref_contrast), 1e-10)
    else:
        assert contrast == 0.0 and ref_contrast == 0.0
    margins.below(f"sp f64 grad {key}", np.abs(g - ref_g).max() / np.abs(ref_g).max(), 1e-9)


@pytest.mark.parametrize("combo", sc.COMBOS, ids=IDS)
def test_f32_kernel_against_the_f64_reference(solver, golden, combo):
    """The yardstick is the reference's own f32 run against its f64 run, from the fixture (never below one f32 rounding, 2^-23);
    the factor 8 covers a different operation order and the device's expf."""
    key = sc.combo_key(combo)
    total, _smooth, _contrast, g = run(solver, combo, np.float32)
    assert g.dtype == np.float32
    ref_total, ref_g = float(golden[f"{key}/total"]), golden[f"{key}/grad"]
    d_total, d_grad = float(golden[f"{key}/delta_total"]), float(golden[f"{key}/delta_grad"])
    margins.below(f"sp f32 total {key}", abs(total - ref_total) / abs(ref_total), 8 * max(d_total, EPS32),
                  info=("reference f32 delta", d_total))
    margins.below(f"sp f32 grad {key}", np.abs(g.astype(np.float64) - ref_g).max() / np.abs(ref_g).max(),
                  8 * max(d_grad, EPS32), info=("reference f32 delta", d_grad))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("combo", [ODD_BOTH, ALIGNED_SECOND], ids=["odd", "aligned"])
def test_results_repeat_bit_for_bit(solver, combo, dtype):
    """No atomics anywhere: values AND gradient repeat bit for bit, on the product build as on the deterministic one; whether
    the gradient is asked for does not change the values."""
    a, b = run(solver, combo, dtype), run(solver, combo, dtype)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.array_equal(a[3], b[3])
    plain = run(solver, combo, dtype, grad=False)
    assert len(plain) == 3 and plain[0] == a[0] and np.array_equal(plain[1], a[1]) and plain[2] == a[2]
    # tables the enabled terms do not read may be passed: they are not read
    contrast_only = (combo[0],) + sc.SETTINGS["contrast"]
    c, d = run(solver, contrast_only, dtype), run(solver, contrast_only, dtype, all_tables=True)
    assert c[0] == d[0] and np.array_equal(c[3], d[3])


def test_frame_wise_split(solver):
    """Contrast alone: the sum runs over the edges of all frames and is divided by F, so the call on all frames of `odd` is the
    mean of the per-frame calls; a frame's gradient is 1 / F of its own call's.  Six positive addends and one division on either
    side, a rounding of 2^-53 each: 1e-15 relative."""
    case = sc.make_case("odd")
    F = case["F"]
    kw = sc.combo_kwargs(ODD_CONTRAST)
    total, smooth, contrast, g = run(solver, ODD_CONTRAST, np.float64)
    assert total == contrast and not smooth.any()
    singles = [solver.spatial_losses(case["depth"][f:f + 1], case["depth_orig"][f:f + 1], frames_per_sample=1, grad=True, **kw)
               for f in range(F)]
    combined = math.fsum(s[0] for s in singles) / F
    margins.below("sp frame-wise split", abs(total - combined) / abs(combined), 1e-15)
    for f in range(F):
        margins.below(f"sp frame-wise gradient {f}", np.abs(g[f] * F - singles[f][3][0]).max() / np.abs(singles[f][3]).max(), 1e-15)


def test_samples_are_means_over_their_frames(solver):
    """`six`: smooth[0] is over six frames; the same table as six samples of one frame gives the six per-frame values, whose mean
    it is."""
    combo = ("six",) + sc.SETTINGS["smooth"]
    case = sc.make_case("six")
    total, smooth, _c, g = run(solver, combo, np.float64)
    total1, smooth1, _c1, g1 = run(solver, combo, np.float64, frames_per_sample=1)
    assert smooth.shape == (1,) and smooth1.shape == (6,) and total == smooth[0]
    margins.below("sp sample mean", abs(smooth[0] - smooth1.mean()) / smooth[0], 1e-14)
    margins.below("sp sample mean total", abs(total - total1) / total, 1e-14)
    margins.below("sp sample mean gradient", np.abs(g - g1).max() / np.abs(g).max(), 1e-14)
    assert case["N"] == 6


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_both_lambdas_zero(solver, dtype):
    case = sc.make_case("odd")
    total, smooth, contrast, g = solver.spatial_losses(np.ascontiguousarray(case["depth"], dtype=dtype), frames_per_sample=2,
                                                       grad=True)
    assert total == 0.0 and contrast == 0.0 and not smooth.any() and g.shape == case["depth"].shape and not g.any()


def test_bad_arguments(solver):
    case = sc.make_case("odd")
    base = dict(sc.case_kwargs(case), **sc.combo_kwargs(ODD_BOTH))
    F, H, W = case["F"], case["H"], case["W"]

    def call(**kw):
        a = dict(base)
        a.update(kw)
        return solver.spatial_losses(**a)
    call()   # the arguments below differ from a call that works by one thing each
    row = lambda a: np.ascontiguousarray(a[..., :1, :])
    col = lambda a: np.ascontiguousarray(a[..., :1])
    bad = [
        ("width and height", lambda: call(depth=row(base["depth"]), depth_orig=row(base["depth_orig"]), image=row(base["image"]))),
        ("width and height", lambda: call(depth=col(base["depth"]), depth_orig=col(base["depth_orig"]), image=col(base["image"]))),
        ("multiple of frames_per_sample", lambda: call(frames_per_sample=4)),
        ("frames_per_sample", lambda: call(frames_per_sample=0)),
        ("sigma_color_grad", lambda: call(sigma_color_grad=0.0)), ("sigma_color_grad", lambda: call(sigma_color_grad=-1.0)),
        ("sigma_color_grad", lambda: call(sigma_color_grad=float("nan"))),
        ("lambda_disparity_smooth", lambda: call(lambda_disparity_smooth=-1.0)),
        ("lambda_contrast_loss", lambda: call(lambda_contrast_loss=float("inf"))),
        ("contrast_thresh", lambda: call(contrast_thresh=float("nan"))),
        ("null depth_orig", lambda: call(depth_orig=None)), ("null image", lambda: call(image=None)),
    ]
    for what, fn in bad:
        with pytest.raises(RuntimeError, match=what):
            fn()
    # a term that is off does not ask for its table or its parameter
    call(image=None, lambda_disparity_smooth=0.0, sigma_color_grad=0.0)
    call(depth_orig=None, lambda_contrast_loss=0.0, contrast_thresh=float("nan"))
    # null pointers and a stale struct_size, through the C entry point; the outputs keep their sentinels: nothing ran
    fn = solver._fn("spatial_losses")
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ptrs = [vp(base["depth"]), vp(base["depth_orig"]), vp(base["image"])]
    total, contrast = C.c_double(-7.0), C.c_double(-7.0)
    smooth = np.full(case["B"], -7.0)
    tail = [C.byref(total), smooth.ctypes.data_as(C.POINTER(C.c_double)), C.byref(contrast), None, None]
    desc = api.spatial_desc(1, F, case["N"], H, W, *ODD_BOTH[1:])
    assert fn(solver._h, C.byref(desc), *ptrs, *tail) == 0 and total.value != -7.0
    total.value = contrast.value = -7.0
    smooth[:] = -7.0
    for k, name in enumerate(("depth", "depth_orig", "image")):
        p = list(ptrs)
        p[k] = None
        assert fn(solver._h, C.byref(desc), *p, *tail) != 0, name
        assert ("null " + name).encode() in solver._lib.cvd_last_error(solver._h)
    for k, name in enumerate(("total", "smooth", "contrast")):
        t = list(tail)
        t[k] = None
        assert fn(solver._h, C.byref(desc), *ptrs, *t) != 0, name
        assert ("null " + name).encode() in solver._lib.cvd_last_error(solver._h)
    assert fn(solver._h, None, *ptrs, *tail) != 0 and b"null desc" in solver._lib.cvd_last_error(solver._h)
    for stale in (desc.struct_size - 8, C.sizeof(api.SpatialDesc), C.sizeof(api.SpatialDesc) | ((api.ABI_REVISION - 1) << 32)):
        d = api.spatial_desc(1, F, case["N"], H, W, *ODD_BOTH[1:])
        d.struct_size = stale
        assert fn(solver._h, C.byref(d), *ptrs, *tail) != 0
        assert b"struct_size" in solver._lib.cvd_last_error(solver._h)
    d = api.spatial_desc(2, F, case["N"], H, W, *ODD_BOTH[1:])
    assert fn(solver._h, C.byref(d), *ptrs, *tail) != 0 and b"precision" in solver._lib.cvd_last_error(solver._h)
    assert total.value == -7.0 and contrast.value == -7.0 and np.all(smooth == -7.0)
    with pytest.raises(ValueError, match="depth_orig"):
        call(depth_orig=base["depth_orig"][:, :-1])
    with pytest.raises(TypeError, match="float32 or float64"):
        call(depth=base["depth"].astype(np.int32))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_torch_modules(dtype):
    """DisparitySmoothLoss, ContrastLoss and JointLoss on GPU tensors, in a fresh process: torch has to be imported before
    libcvd_hip.so is loaded (the process then holds one HIP runtime, torch's), which a test in the middle of the suite cannot
    arrange.  The checks are tests/spatial_torch_child.py's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.spatial_torch_child", dtype], cwd=root, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "torch modules ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
