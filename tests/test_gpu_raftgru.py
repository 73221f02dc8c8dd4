"""GPU checks of the SepConvGRU kernels (robust_cvd_amd/csrc/cvd_raftgru.h) through the array path
(Solver.raft_sepconv_gru) and, in a fresh process, through the torch drop-in robust_cvd_amd.raft_ops.SepConvGRU
(tests/raftgru_torch_child.py).

Bar: |kernel - f64| <= 8 x max(delta, 2^-23 x scale) against the float64 restatement (tests/raftgru_reference.py), delta = the
REFERENCE's own f32 error against that restatement for the case and scale = the largest |output|, both read from the fixture
(tests/golden/reference_py/raftgru_golden.npz, minted on the CPU; never from this kernel); against the reference's stored f32
values that bar + delta.  The factor 8 is the one the project's other f32 kernels carry (tests/test_gpu_raftops.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import margins
from tests import raftgru_cases as gc
from tests import raftgru_reference as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from robust_cvd_amd.api import Solver
    return Solver(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(gr.GOLDEN)


def run(solver, case, x=None):
    return solver.raft_sepconv_gru(case["h"], case["x"] if x is None else x, case["weights"], case["biases"])


@pytest.fixture(scope="module")
def results(solver):
    """Per case: (inputs, f64 restatement, kernel output): computed once, shared, left unchanged."""
    out = {}
    for name in gc.CASES:
        case = gc.make_case(name)
        out[name] = (case, gr.sepconv_gru(case["h"], case["x"], case["weights"], case["biases"]), run(solver, case))
    return out


@pytest.mark.parametrize("name", list(gc.CASES))
def test_against_the_restatement_and_the_reference(results, golden, name):
    case, want, got = results[name]
    assert gc.input_digest(case) == golden[name + "/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    assert got.shape == case["h"].shape and got.dtype == np.float32 and np.isfinite(got).all()
    delta = float(golden[name + "/delta"])
    bar = gr.bar(delta, golden[name + "/scale"])
    err = np.abs(got - want).max()
    print(f"{name}: max |kernel - f64| {err:.3e}, bar {bar:.3e} (reference's own delta {delta:.3e})")
    margins.below(f"raft gru {name}", err, bar)
    margins.below(f"raft gru {name} vs reference", np.abs(gc.sample_view(case, got) - golden[name + "/out"]).max(), bar + delta)


def test_segment_forms_give_the_same_bits(solver, results):
    for name in ("5x7b3", "2x130"):
        case, _want, got = results[name]
        x = case["x"]
        assert np.array_equal(run(solver, case, (x[:, :128], x[:, 128:])), got)
        assert np.array_equal(run(solver, case, (x[:, :32], x[:, 32:128], x[:, 128:])), got)
        assert np.array_equal(run(solver, case, [x]), got)


def test_results_repeat_bit_for_bit(solver, results):
    for name in ("9x11", "131x2"):
        case, _want, got = results[name]
        assert np.array_equal(run(solver, case), got)


def test_a_batch_is_its_images_one_by_one(solver, results):
    """B = 3 in one tile of 64 pixels against three calls at B = 1: no pixel of a neighbouring image is read as halo."""
    case, _want, got = results["5x7b3"]
    for b in range(3):
        one = solver.raft_sepconv_gru(case["h"][b:b + 1], case["x"][b:b + 1], case["weights"], case["biases"])
        assert np.array_equal(one[0], got[b]), b


def test_pm100_is_exact_where_planted(results):
    case, _want, got = results["pm100"]
    assert np.array_equal(got[:, list(gc.PM100_KEEPS_H)], case["h"][:, list(gc.PM100_KEEPS_H)])     # z = 0 in both halves: h itself
    assert (got[:, list(gc.PM100_PLUS_ONE)] == 1.0).all()                                             # z = 1, q = tanh(+100)
    assert (got[:, list(gc.PM100_MINUS_ONE)] == -1.0).all()


def _hip():
    from robust_cvd_amd import api
    return api._hip_runtime()


def test_refusals(solver):
    case = gc.make_case("3x2")
    h, x, w, b = case["h"], case["x"], case["weights"], case["biases"]
    _hip().hipGetLastError()      # (the runtime keeps the last error of the thread until it is asked for)
    refused = [
        (TypeError, lambda: solver.raft_sepconv_gru(h.astype(np.float64), x, w, b)),
        (TypeError, lambda: solver.raft_sepconv_gru(h, x.astype(np.float16), w, b)),
        (TypeError, lambda: solver.raft_sepconv_gru(h, x, w, [a.astype(np.float64) for a in b])),
        (ValueError, lambda: solver.raft_sepconv_gru(h[:, :96], x, w, b)),
        (ValueError, lambda: solver.raft_sepconv_gru(h, x[:, :192], w, b)),
        (ValueError, lambda: solver.raft_sepconv_gru(h, (x[:, :100], x[:, 100:]), w, b)),
        (ValueError, lambda: solver.raft_sepconv_gru(h, (x[:, :64],) * 4, w, b)),
        (ValueError, lambda: solver.raft_sepconv_gru(h, x[:, :, :2], w, b)),
        (ValueError, lambda: solver.raft_sepconv_gru(h[:0], x[:0], w, b)),
        (ValueError, lambda: solver.raft_sepconv_gru(h, x, w[::-1], b)),
        (ValueError, lambda: solver.raft_sepconv_gru(h, x, w[:5], b[:5])),
    ]
    for exc, call in refused:
        with pytest.raises(exc):
            call()
    assert _hip().hipDeviceSynchronize() == 0 and _hip().hipGetLastError() == 0


def test_the_entry_point_refuses_too(solver):
    """The C ABI's own checks (a caller that bypasses the Python layer): an error that names the value, no launch, and the next
    good call works."""
    import ctypes as C
    p = C.c_void_p(4096)       # never dereferenced: every call below is rejected before any device work
    six = (C.c_void_p * 6)(*([4096] * 6))

    def call(B=1, H=3, W=2, hidden=p, nseg=1, segs=(8192,), chans=(256,), weights=six, biases=six, out=C.c_void_p(1 << 20)):
        return solver._fn("raft_sepconv_gru_device")(solver._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), hidden, C.c_int32(nseg),
                                                     (C.c_void_p * len(segs))(*segs), (C.c_int32 * len(chans))(*chans), weights,
                                                     biases, out, None)
    _hip().hipGetLastError()
    cases = [(dict(B=0), ">= 1"), (dict(W=0), ">= 1"),
             (dict(nseg=0), "num_segments"), (dict(nseg=4, segs=(8192,) * 4, chans=(64,) * 4), "num_segments"),
             (dict(nseg=2, segs=(8192, 65536), chans=(100, 156)), "multiple of 32"),
             (dict(chans=(224,)), "input_dim"),
             (dict(hidden=None), "null"),
             (dict(weights=(C.c_void_p * 6)(4096, 4096, 4100, 4096, 4096, 4096)), "aligned"),
             (dict(out=p), "aliases h"),
             (dict(out=C.c_void_p(8192 + 64)), "aliases segment 0")]
    for kwargs, word in cases:
        with pytest.raises(RuntimeError, match=word):
            solver._check(call(**kwargs))
    assert _hip().hipDeviceSynchronize() == 0 and _hip().hipGetLastError() == 0
    case = gc.make_case("1x1")
    assert np.isfinite(run(solver, case)).all()


def test_torch_module():
    """robust_cvd_amd.raft_ops.SepConvGRU on GPU tensors, in a fresh process: torch has to be imported before libcvd_hip.so is
    loaded.  The checks are tests/raftgru_torch_child.py's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.raftgru_torch_child"], cwd=root, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "raft gru torch module ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
