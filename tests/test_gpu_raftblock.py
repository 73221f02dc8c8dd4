"""GPU checks of the update block's convolution kernel and of the block (robust_cvd_amd/csrc/cvd_raftconv.h)
through the array paths (Solver.raft_conv2d, Solver.raft_update_block) and, in a fresh process, through the torch drop-in
robust_cvd_amd.raft_ops.BasicUpdateBlock (tests/raftblock_torch_child.py).

Bar: |kernel - f64| <= 8 x max(delta, 2^-23 x scale) against the float64 restatement (tests/raftblock_reference.py), delta = the
REFERENCE's own f32 error against that restatement for the case and output, scale = the largest |output|, both read from the
fixture (tests/golden/reference_py/raftblock_golden.npz, minted on the CPU; never from this kernel); against the reference's stored
f32 values that bar + delta.  The factor 8 is the one the project's other f32 kernels carry (tests/test_gpu_raftgru.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import margins
from tests import raftblock_cases as bc
from tests import raftblock_reference as br

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from robust_cvd_amd.api import Solver
    return Solver(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(br.GOLDEN)


def run_conv(solver, case, x=None):
    """The case through Solver.raft_conv2d: the N written channels, and the whole output tensor (prefilled with SENTINEL)."""
    x = bc.split(case) if x is None else x
    w, b = case["weights"], case["biases"]
    B, _, H, W = case["x"].shape
    N = sum(a.shape[0] for a in w)
    total, first = case["window"] or (N, 0)
    out = np.full((B, total, H, W), bc.SENTINEL, np.float32)
    full = solver.raft_conv2d(x if len(x) > 1 else x[0], w if len(w) > 1 else w[0], b if len(b) > 1 else b[0], relu=case["relu"],
                              scale=case["scale"], out=out, out_first=first)
    return full[:, first:first + N], full


def run_block(solver, case, **kwargs):
    return solver.raft_update_block(case["net"], case["inp"], case["corr"], case["flow"], case["weights"], case["biases"], **kwargs)


def chain(solver, case, compute_mask=True):
    """The block's stages one by one through raft_conv2d and raft_sepconv_gru, as cvd_raft_update_block_device chains them:
    -> (net, mask, delta_flow), dict of the intermediates."""
    w, b = case["weights"], case["biases"]
    B, _, H, W = case["net"].shape
    cor1 = solver.raft_conv2d(case["corr"], w[0], b[0], relu=True)
    cor_flo = np.full((B, 256, H, W), bc.SENTINEL, np.float32)
    cor_flo = solver.raft_conv2d(cor1, w[1], b[1], relu=True, out=cor_flo, out_first=0)
    flo1 = solver.raft_conv2d(case["flow"], w[2], b[2], relu=True)
    cor_flo = solver.raft_conv2d(flo1, w[3], b[3], relu=True, out=cor_flo, out_first=192)
    motion = np.full((B, 128, H, W), bc.SENTINEL, np.float32)
    motion = solver.raft_conv2d(cor_flo, w[4], b[4], relu=True, out=motion, out_first=0)
    assert (motion[:, 126:] == bc.SENTINEL).all()
    motion[:, 126:] = case["flow"]
    net = solver.raft_sepconv_gru(case["net"], (case["inp"], motion), w[5:11], b[5:11])
    flow_hidden = solver.raft_conv2d(net, w[11], b[11], relu=True)
    delta_flow = solver.raft_conv2d(flow_hidden, w[12], b[12])
    kept = {"cor1": cor1, "cor_flo": cor_flo, "flo1": flo1, "motion_features": motion, "flow_hidden": flow_hidden}
    mask = None
    if compute_mask:
        kept["mask_hidden"] = solver.raft_conv2d(net, w[13], b[13], relu=True)
        mask = solver.raft_conv2d(kept["mask_hidden"], w[14], b[14], scale=0.25)
    return (net, mask, delta_flow), kept


@pytest.fixture(scope="module")
def conv_results(solver):
    """Per single-convolution case: (inputs, f64 restatement, kernel output window, whole output tensor): computed once, shared."""
    out = {}
    for name in bc.CONV_CASES:
        case = bc.make_conv_case(name)
        out[name] = (case, br.conv_case(case)) + run_conv(solver, case)
    return out


@pytest.fixture(scope="module")
def block_results(solver):
    """Per block case: (inputs, f64 restatement (net, mask, delta_flow), kernel outputs): computed once, shared."""
    out = {}
    for name in bc.BLOCK_CASES:
        case = bc.make_block_case(name)
        out[name] = (case, br.block_case(case), run_block(solver, case))
    return out


def check(label, key, golden, case, o, got, want):
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    delta = float(golden[f"{key}/{o}_delta"])
    bar = br.bar(delta, golden[f"{key}/{o}_scale"])
    err = np.abs(got - want).max()
    print(f"{key} {o}: max |kernel - f64| {err:.3e}, bar {bar:.3e}, share {err / bar:.3f} (reference's own delta {delta:.3e})")
    margins.below(f"{label} {o}", err, bar)
    margins.below(f"{label} {o} vs reference", np.abs(bc.sample_view(case, got) - golden[f"{key}/{o}"]).max(), bar + delta)


@pytest.mark.parametrize("name", list(bc.CONV_CASES))
def test_convolution_against_the_restatement_and_the_reference(conv_results, golden, name):
    case, want, got, full = conv_results[name]
    assert bc.input_digest(case) == golden[f"conv/{name}/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    check(f"raft conv {name}", "conv/" + name, golden, case, "out", got, want)
    if case["window"]:
        total, first = case["window"]
        outside = np.r_[0:first, first + got.shape[1]:total]
        assert len(outside) and (full[:, outside] == bc.SENTINEL).all(), "a channel outside the output window was written"


@pytest.mark.parametrize("name", list(bc.BLOCK_CASES))
def test_block_against_the_restatement_and_the_reference(block_results, golden, name):
    case, want, got = block_results[name]
    assert bc.input_digest(case) == golden[f"block/{name}/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    for o, g, w in zip(bc.OUTPUTS, got, want):
        check(f"raft block {name}", "block/" + name, golden, case, o, g, w)


def test_segment_forms_give_the_same_bits(solver, conv_results):
    for name in ("c3seg_3x5x7", "c3seg_1x2x130"):
        case, _want, got, _full = conv_results[name]
        x = case["x"]
        assert np.array_equal(run_conv(solver, case, (x,))[0], got)
        assert np.array_equal(run_conv(solver, case, (x[:, :64], x[:, 64:192], x[:, 192:]))[0], got)
        assert np.array_equal(run_conv(solver, case, (x[:, :128], x[:, 128:]))[0], got)
    # two stacked weight tensors against one launch each
    case, _want, got, _full = conv_results["c3x2_2x9x11"]
    for i in range(2):
        one = solver.raft_conv2d(case["x"], case["weights"][i], case["biases"][i], relu=True)
        assert np.array_equal(one, got[:, 256 * i:256 * (i + 1)])


def test_results_repeat_bit_for_bit(solver, conv_results, block_results):
    for name in ("c1_3x5x7", "c7_2x9x11", "c3n2_3x5x7"):
        case, _want, got, _full = conv_results[name]
        assert np.array_equal(run_conv(solver, case)[0], got)
    case, _want, got = block_results["9x11"]
    for a, b in zip(run_block(solver, case), got):
        assert np.array_equal(a, b)


def test_a_batch_is_its_images_one_by_one(solver, conv_results, block_results):
    """B = 3 (105 pixels: one tile of 64 straddles every row and all three images) against three calls at B = 1: no pixel of a
    neighbouring image is read as halo."""
    for name in ("c1_3x5x7", "c3seg_3x5x7", "c3n2_3x5x7"):
        case, _want, got, _full = conv_results[name]
        for i in range(3):
            assert np.array_equal(run_conv(solver, dict(case, x=case["x"][i:i + 1]))[0][0], got[i]), (name, i)
    case, _want, got = block_results["5x7b3"]
    for i in range(3):
        one = run_block(solver, dict(case, **{k: case[k][i:i + 1] for k in ("net", "inp", "corr", "flow")}))
        for a, b in zip(one, got):
            assert np.array_equal(a[0], b[i]), i


def test_the_fused_scale_is_a_separate_multiply(solver, conv_results):
    case, _want, got, _full = conv_results["c1s_1x4x6"]
    plain = solver.raft_conv2d(case["x"], case["weights"][0], case["biases"][0], scale=1.0)
    assert np.array_equal(np.float32(0.25) * plain, got)


@pytest.mark.parametrize("name", ["9x11", "5x7b3", "planted"])
def test_the_block_is_its_stages_chained(solver, block_results, name):
    """raft_update_block against the same stages through raft_conv2d and raft_sepconv_gru, bit for bit: scratch aliasing and
    channel-window mistakes apart from numerics."""
    case, _want, got = block_results[name]
    outs, _kept = chain(solver, case)
    for o, a, b in zip(bc.OUTPUTS, outs, got):
        assert np.array_equal(a, b), o


def test_without_the_mask(solver, block_results):
    for name in ("9x11", "2x130"):
        case, _want, got = block_results[name]
        net, mask, delta_flow = run_block(solver, case, compute_mask=False)
        assert mask is None and np.array_equal(net, got[0]) and np.array_equal(delta_flow, got[2])


def test_planted_is_exact(solver, block_results):
    case, _want, got = block_results["planted"]
    (_net, mask, delta_flow), kept = chain(solver, case)
    tensors = dict(kept, mask=mask, delta_flow=delta_flow)
    where = {"encoder.convc1": ("cor1", 0), "encoder.convc2": ("cor_flo", 0), "encoder.convf1": ("flo1", 0),
             "encoder.convf2": ("cor_flo", 192), "encoder.conv": ("motion_features", 0), "flow_head.conv1": ("flow_hidden", 0),
             "flow_head.conv2": ("delta_flow", 0), "mask.0": ("mask_hidden", 0), "mask.2": ("mask", 0)}
    for layer, (zeroed, minus) in bc.PLANTED.items():
        tensor, first = where[layer]
        for ch, value in zeroed.items():
            b = np.float32(value)
            want = {"flow_head.conv2": b, "mask.2": np.float32(0.25) * b}.get(layer, max(b, np.float32(0.0)))
            assert (tensors[tensor][:, first + ch] == want).all(), (layer, ch)
        for ch in minus:
            assert (tensors[tensor][:, first + ch] == 0.0).all(), (layer, ch)
    # ... and in the block call's own outputs
    for ch, value in bc.PLANTED["mask.2"][0].items():
        assert (got[1][:, ch] == np.float32(0.25) * np.float32(value)).all(), ch
    assert (got[2][:, 1] == np.float32(bc.PLANTED["flow_head.conv2"][0][1])).all()


def _hip():
    from robust_cvd_amd import api
    return api._hip_runtime()


def test_refusals(solver):
    case = bc.make_block_case("3x2")
    a = [case[k] for k in ("net", "inp", "corr", "flow")]
    w, b = case["weights"], case["biases"]
    conv = bc.make_conv_case("c3seg_1x3x2")
    x, cw, cb = conv["x"], conv["weights"][0], conv["biases"][0]
    _hip().hipGetLastError()      # (the runtime keeps the last error of the thread until it is asked for)
    refused = [
        (TypeError, lambda: solver.raft_update_block(a[0].astype(np.float64), a[1], a[2], a[3], w, b)),
        (TypeError, lambda: solver.raft_update_block(a[0], a[1], a[2].astype(np.float16), a[3], w, b)),
        (TypeError, lambda: solver.raft_update_block(*a, w, [v.astype(np.float64) for v in b])),
        (ValueError, lambda: solver.raft_update_block(a[0][:, :96], *a[1:], w, b)),
        (ValueError, lambda: solver.raft_update_block(a[0], a[1], a[2][:, :196], a[3], w, b)),
        (ValueError, lambda: solver.raft_update_block(a[0], a[1], a[2], a[3][:, :, :2], w, b)),
        (ValueError, lambda: solver.raft_update_block(*(v[:0] for v in a), w, b)),
        (ValueError, lambda: solver.raft_update_block(*a, w[::-1], b)),
        (ValueError, lambda: solver.raft_update_block(*a, w[:14], b[:14])),
        (TypeError, lambda: solver.raft_conv2d(x.astype(np.float64), cw, cb)),
        (ValueError, lambda: solver.raft_conv2d(x, np.zeros((126, 256, 5, 5), np.float32), cb)),
        (ValueError, lambda: solver.raft_conv2d((x[:, :100], x[:, 100:]), cw, cb)),
        (ValueError, lambda: solver.raft_conv2d((x[:, :64],) * 4, cw, cb)),
        (ValueError, lambda: solver.raft_conv2d(x[:, :192], cw, cb)),
        (ValueError, lambda: solver.raft_conv2d(x[:0], cw, cb)),
        (ValueError, lambda: solver.raft_conv2d(x, [cw, cw], [cb, cb])),
        (ValueError, lambda: solver.raft_conv2d(x, cw, cb, out=np.zeros((1, 128, 3, 2), np.float32), out_first=3)),
    ]
    for exc, call in refused:
        with pytest.raises(exc):
            call()
    assert _hip().hipDeviceSynchronize() == 0 and _hip().hipGetLastError() == 0


def test_the_entry_points_refuse_too(solver):
    """The C ABI's own checks (a caller that bypasses the Python layer): an error that names the value, no launch, and the next
    good call works."""
    import ctypes as C
    p = 1 << 20                # never dereferenced: every call below is rejected before any device work

    def conv(B=1, H=3, W=2, nseg=1, segs=(2 * p,), chans=(256,), nw=1, weights=(3 * p,), biases=(4 * p,), cin=256, cout=126, k=3,
             stride=1, dilation=1, groups=1, act=1, out=5 * p, total=128, first=0):
        return solver._fn("raft_conv2d_device")(
            solver._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(nseg), (C.c_void_p * len(segs))(*segs),
            (C.c_int32 * len(chans))(*chans), C.c_int32(nw), (C.c_void_p * len(weights))(*weights), (C.c_void_p * len(biases))(*biases),
            C.c_int32(cin), C.c_int32(cout), C.c_int32(k), C.c_int32(stride), C.c_int32(dilation), C.c_int32(groups), C.c_int32(act),
            C.c_float(1.0), C.c_void_p(out), C.c_int32(total), C.c_int32(first), None)

    fifteen = (C.c_void_p * 15)(*([16 * p] * 15))

    def block(B=1, H=3, W=2, cc=324, planes=324, net=2 * p, inp=3 * p, corr=4 * p, flow=5 * p, weights=fifteen, biases=fifteen,
              net_out=6 * p, delta=7 * p, mask=8 * p):
        return solver._fn("raft_update_block_device")(
            solver._h, C.c_int32(B), C.c_int32(H), C.c_int32(W), C.c_int32(cc), C.c_int32(planes), C.c_void_p(net), C.c_void_p(inp),
            C.c_void_p(corr), C.c_void_p(flow), weights, biases, C.c_void_p(net_out), C.c_void_p(delta), C.c_void_p(mask), None)

    _hip().hipGetLastError()
    cases = [(conv, dict(B=0), ">= 1"), (conv, dict(W=0), ">= 1"),
             (conv, dict(k=5), "kernel_size must be 1, 3 or 7"), (conv, dict(k=2), "kernel_size"),
             (conv, dict(stride=2), "stride must be 1"), (conv, dict(dilation=2), "dilation must be 1"),
             (conv, dict(groups=2), "groups must be 1"), (conv, dict(act=2), "activation"),
             (conv, dict(nseg=0), "num_segments"), (conv, dict(nseg=4, segs=(2 * p,) * 4, chans=(64,) * 4), "num_segments"),
             (conv, dict(nseg=2, segs=(2 * p, 2 * p + 65536), chans=(100, 156)), "multiple of 32"),
             (conv, dict(chans=(224,)), "in_channels is 256"),
             (conv, dict(segs=(None,)), "null"), (conv, dict(out=None), "null"), (conv, dict(weights=(None,)), "null"),
             (conv, dict(nw=2, weights=(3 * p, 3 * p), biases=(4 * p, 4 * p)), "multiples of 64"),
             (conv, dict(first=3), "exceeds the tensor's 128"), (conv, dict(total=100), "exceeds the tensor's 100"),
             (conv, dict(first=-1), "exceeds"),
             (conv, dict(out=2 * p + 64), "overlaps segment 0"),
             (block, dict(H=0), ">= 1"), (block, dict(cc=196), "corr has 196 channels, encoder.convc1 takes 324"),
             (block, dict(net=None), "null"), (block, dict(delta=None), "null"),
             (block, dict(net_out=2 * p), "net_out overlaps net"), (block, dict(mask=4 * p + 128), "mask overlaps corr"),
             (block, dict(delta=6 * p + 8), "overlaps"),
             (block, dict(weights=(C.c_void_p * 15)(*([16 * p] * 7 + [16 * p + 4] + [16 * p] * 7))), "aligned")]
    for fn, kwargs, word in cases:
        with pytest.raises(RuntimeError, match=word):
            solver._check(fn(**kwargs))
    assert _hip().hipDeviceSynchronize() == 0 and _hip().hipGetLastError() == 0
    case = bc.make_block_case("1x1")
    assert all(np.isfinite(o).all() for o in run_block(solver, case))


def test_torch_module():
    """robust_cvd_amd.raft_ops.BasicUpdateBlock on GPU tensors, in a fresh process: torch has to be imported before libcvd_hip.so
    is loaded.  The checks are tests/raftblock_torch_child.py's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.raftblock_torch_child"], cwd=root, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "raft block torch module ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
