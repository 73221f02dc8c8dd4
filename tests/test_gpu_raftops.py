"""GPU checks of the RAFT operators (robust_cvd_amd/csrc/cvd_raftops.h) through the array path
(Solver.raft_corr_pyramid / raft_corr_lookup / raft_upsample_flow) and, in a fresh process, through the torch drop-ins of
robust_cvd_amd.raft_ops (tests/raftops_torch_child.py).

Bars: level 0 of the pyramid equals raw / f32(sqrt(f32(dim))) bit for bit.  Pooled levels, lookup and upsampling are held against
the float64 restatement (tests/raftops_reference.py): |kernel - f64| <= 8 x max(delta, 2^-23 x scale), delta = the REFERENCE's own
f32 error against that restatement for the case and scale = the largest |value|, both read from the fixture
(tests/golden/reference_py/raftops_golden.npz, minted on the CPU; never from this kernel).  The factor 8 is the one the project's
other f32 kernels carry (tests/consistency_torch_child.py); it covers that the lookup rounds ONE shared pair of fractions per query
and level where torch rounds every tap through its own normalise / unnormalise round trip."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import margins
from tests import raftops_cases as rc
from tests import raftops_reference as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from robust_cvd_amd.api import Solver
    return Solver(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(rr.GOLDEN)


@pytest.fixture(scope="module")
def corr(solver):
    """Per case: (inputs, f64 pyramid, f64 lookup, kernel pyramid, kernel lookup): computed once, shared, left unchanged."""
    out = {}
    for name in rc.CORR:
        case = rc.make_corr_case(name)
        pyr64 = rr.pyramid(case["raw"], case["dim"], case["levels"])
        look64 = rr.lookup(pyr64, case["coords"], case["r"])
        pyr = solver.raft_corr_pyramid(case["raw"], case["dim"], case["levels"])
        look = solver.raft_corr_lookup(pyr, case["coords"], case["r"])
        out[name] = (case, pyr64, look64, pyr, look)
    return out


@pytest.mark.parametrize("name", list(rc.CORR))
def test_level0_is_the_f32_quotient_bit_for_bit(corr, golden, name):
    case, _pyr64, _look64, pyr, _look = corr[name]
    assert rc.input_digest(case) == golden[name + "/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    assert pyr[0].dtype == np.float32 and pyr[0].shape == case["raw"].shape
    assert np.array_equal(pyr[0], case["raw"] / np.float32(np.sqrt(np.float32(case["dim"]))))
    if name == "square16":
        assert not np.array_equal(pyr[0], case["raw"] * np.float32(1.0 / np.sqrt(np.float32(48))))    # (the case tells the two apart)


@pytest.mark.parametrize("name", list(rc.CORR))
def test_pooled_levels(corr, golden, name):
    case, pyr64, _look64, pyr, _look = corr[name]
    assert len(pyr) == case["levels"]
    bar = rr.bar(golden[name + "/delta_pyr"], golden[name + "/scale_pyr"])
    for l in range(1, case["levels"]):
        assert pyr[l].shape == (len(case["raw"]), case["h"] >> l, case["w"] >> l) and pyr[l].dtype == np.float32
        err = np.abs(pyr[l] - pyr64[l]).max()
        print(f"{name} level {l}: max |kernel - f64| {err:.3e}, bar {bar:.3e}")
        margins.below(f"raft pyramid {name} level {l}", err, bar)
        # ... and the reference's stored f32 values of the sampled queries, within both f32 errors
        margins.below(f"raft pyramid {name} level {l} vs reference", np.abs(pyr[l][case["queries"]] - golden[f"{name}/pyr{l}"]).max(),
                      bar + float(golden[name + "/delta_pyr"]))


@pytest.mark.parametrize("name", list(rc.CORR))
def test_lookup(corr, golden, name):
    case, _pyr64, look64, _pyr, look = corr[name]
    n = 2 * case["r"] + 1
    assert look.shape == (case["B"], case["levels"] * n * n, case["h"], case["w"]) and look.dtype == np.float32
    bar = rr.bar(golden[name + "/delta_lookup"], golden[name + "/scale_lookup"])
    err = np.abs(look - look64).max()
    print(f"{name} lookup: max |kernel - f64| {err:.3e}, bar {bar:.3e} (reference's own delta {float(golden[name + '/delta_lookup']):.3e})")
    margins.below(f"raft lookup {name}", err, bar)
    margins.below(f"raft lookup {name} vs reference", np.abs(rc.query_view(case, look) - golden[name + "/lookup"]).max(),
                  bar + float(golden[name + "/delta_lookup"]))
    # the planted outside and huge coordinates: exact zeros, on every level
    flat = look.transpose(0, 2, 3, 1).reshape(len(case["raw"]), -1)
    assert not flat[list(rc.ZERO_CELLS)].any()
    assert flat[:7].any(axis=1).all()


def test_lookup_with_fewer_levels_and_each_radius(solver, corr):
    """Runtime level count and radius: a prefix of the pyramid at radius 1 and 2 against the restatement (the bar of the case:
    the same maps and coordinates, fewer taps)."""
    g = np.load(rr.GOLDEN)
    case, pyr64, _look64, pyr, _look = corr["odd17x23"]
    bar = rr.bar(g["odd17x23/delta_lookup"], g["odd17x23/scale_lookup"])
    for levels, radius in ((1, 1), (2, 2)):
        got = solver.raft_corr_lookup(pyr[:levels], case["coords"], radius)
        want = rr.lookup(pyr64[:levels], case["coords"], radius)
        assert got.shape == want.shape
        margins.below(f"raft lookup odd17x23 levels {levels} radius {radius}", np.abs(got - want).max(), bar)


@pytest.mark.parametrize("name", list(rc.UPSAMPLE))
def test_upsampling(solver, golden, name):
    case = rc.make_upsample_case(name)
    assert rc.input_digest(case) == golden[name + "/input_sha256"].tobytes().decode()
    up = solver.raft_upsample_flow(case["flow"], case["mask"])
    want = rr.upsample(case["flow"], case["mask"])
    assert up.shape == want.shape and up.dtype == np.float32 and np.isfinite(up).all()
    bar = rr.bar(golden[name + "/delta"], golden[name + "/scale"])
    err = np.abs(up - want).max()
    print(f"{name}: max |kernel - f64| {err:.3e}, bar {bar:.3e}")
    margins.below(f"raft upsampling {name}", err, bar)
    margins.below(f"raft upsampling {name} vs reference", np.abs(up - golden[name + "/out"]).max(), bar + float(golden[name + "/delta"]))
    assert np.array_equal(up, solver.raft_upsample_flow(case["flow"], case["mask"]))     # repeats bit for bit


def test_results_repeat_bit_for_bit(solver, corr):
    for name, (case, _p64, _l64, pyr, look) in corr.items():
        again = solver.raft_corr_pyramid(case["raw"], case["dim"], case["levels"])
        assert all(np.array_equal(a, b) for a, b in zip(pyr, again))
        assert np.array_equal(look, solver.raft_corr_lookup(again, case["coords"], case["r"]))


def _hip():
    from robust_cvd_amd import api
    return api._hip_runtime()


def _forget_earlier_errors():
    _hip().hipGetLastError()      # (the runtime keeps the last error of the thread until it is asked for)


def _no_device_error():
    assert _hip().hipDeviceSynchronize() == 0 and _hip().hipGetLastError() == 0


def test_refusals(solver):
    case = rc.make_corr_case("square16")
    raw, coords = case["raw"], case["coords"]
    pyr = [np.zeros((256, 16 >> l, 16 >> l), np.float32) for l in range(4)]
    up = rc.make_upsample_case("up1x1")
    _forget_earlier_errors()
    refused = [
        (ValueError, lambda: solver.raft_corr_pyramid(raw[:, :8, :8], 48, 4)),        # coarsest level 1 x 1
        (ValueError, lambda: solver.raft_corr_pyramid(raw[:, :, :15], 48, 4)),        # ... 2 x 1
        (ValueError, lambda: solver.raft_corr_pyramid(raw, 48, 5)),
        (ValueError, lambda: solver.raft_corr_pyramid(raw, 48, 0)),
        (ValueError, lambda: solver.raft_corr_pyramid(raw, 0, 4)),
        (ValueError, lambda: solver.raft_corr_pyramid(raw[0], 48, 4)),
        (TypeError, lambda: solver.raft_corr_pyramid(raw.astype(np.float64), 48, 4)),
        (TypeError, lambda: solver.raft_corr_pyramid(raw.astype(np.float16), 48, 4)),
        (ValueError, lambda: solver.raft_corr_lookup(pyr, coords, 0)),
        (ValueError, lambda: solver.raft_corr_lookup(pyr, coords, 5)),
        (ValueError, lambda: solver.raft_corr_lookup(pyr + [np.zeros((256, 1, 1), np.float32)], coords, 4)),
        (ValueError, lambda: solver.raft_corr_lookup([a[:, :8, :8] for a in pyr[:2]] + [np.zeros((256, 2, 2), np.float32),
                                                                                       np.zeros((256, 1, 1), np.float32)], coords, 4)),
        (ValueError, lambda: solver.raft_corr_lookup(pyr, coords[:, :, :8], 4)),        # 128 queries, 256 maps
        (ValueError, lambda: solver.raft_corr_lookup([pyr[0], pyr[1][:, :7]], coords, 4)),
        (TypeError, lambda: solver.raft_corr_lookup(pyr, coords.astype(np.float64), 4)),
        (ValueError, lambda: solver.raft_upsample_flow(up["flow"], up["mask"][:, :575])),
        (ValueError, lambda: solver.raft_upsample_flow(up["flow"][:, :1], up["mask"])),
        (TypeError, lambda: solver.raft_upsample_flow(up["flow"].astype(np.float64), up["mask"])),
    ]
    for exc, call in refused:
        with pytest.raises(exc):
            call()
    _no_device_error()


def test_the_entry_points_refuse_too(solver):
    """The C ABI's own checks (a caller that bypasses the Python layer): an error that names the value, no launch, and the next
    good call works."""
    import ctypes as C
    table = (C.c_void_p * 4)(16, 16, 16, 16)      # never dereferenced: every call below is rejected before any device work
    p = C.c_void_p(16)
    _forget_earlier_errors()
    calls = [("raft_corr_pyramid_device", (C.c_int64(4), C.c_int32(8), C.c_int32(8), C.c_int32(48), C.c_int32(4), p, table, None), "2 x 2"),
             ("raft_corr_pyramid_device", (C.c_int64(4), C.c_int32(16), C.c_int32(16), C.c_int32(48), C.c_int32(5), p, table, None), "num_levels"),
             ("raft_corr_pyramid_device", (C.c_int64(4), C.c_int32(16), C.c_int32(16), C.c_int32(48), C.c_int32(4), C.c_void_p(20), table, None), "aligned"),
             ("raft_corr_lookup_device", (C.c_int32(1), C.c_int32(2), C.c_int32(2), C.c_int32(16), C.c_int32(16), C.c_int32(4), C.c_int32(5), table, p, p, None), "radius"),
             ("raft_corr_lookup_device", (C.c_int32(1), C.c_int32(2), C.c_int32(2), C.c_int32(16), C.c_int32(16), C.c_int32(4), C.c_int32(4), table, None, p, None), "null"),
             ("raft_upsample_flow_device", (C.c_int32(0), C.c_int32(2), C.c_int32(2), p, p, p, None), ">= 1")]
    for name, args, word in calls:
        with pytest.raises(RuntimeError, match=word):
            solver._check(solver._fn(name)(solver._h, *args))
    _no_device_error()
    case = rc.make_upsample_case("up1x1")
    assert np.isfinite(solver.raft_upsample_flow(case["flow"], case["mask"])).all()


def test_torch_module():
    """robust_cvd_amd.raft_ops.CorrBlock / upsample_flow on GPU tensors, in a fresh process: torch has to be imported before
    libcvd_hip.so is loaded.  The checks are tests/raftops_torch_child.py's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.raftops_torch_child"], cwd=root, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "raft torch module ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
