"""float64 numpy restatement of the reference's SepConvGRU.forward (raft/core/update.py:37-75) for
robust_cvd_amd/csrc/cvd_raftgru.h, and the bar of the GPU tests.  The mathematics in double, from the f32 inputs; the fixture
(raftgru_golden.npz, minted by tests/golden/reference_py/make_raftgru_golden.py) records how far the reference's own f32
arithmetic is from it."""
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "raftgru_golden.npz")
EPS32 = 2.0 ** -23


def _conv(inp, weight, bias, axis):
    """inp [B, C, H, W] f64; weight [O, C, 5] taps along `axis` (3: a row, 2: a column), zero padding of 2; -> [B, O, H, W]."""
    pad = [(0, 0)] * 4
    pad[axis] = (2, 2)
    padded = np.pad(inp, pad)
    n = inp.shape[axis]
    out = np.zeros((inp.shape[0], weight.shape[0]) + inp.shape[2:], np.float64)
    for t in range(5):
        idx = [slice(None)] * 4
        idx[axis] = slice(t, t + n)
        out += np.einsum("oc,bchw->bohw", weight[:, :, t], padded[tuple(idx)])
    return out + bias.reshape(1, -1, 1, 1)


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def sepconv_gru(h, x, weights, biases, details=False):
    """h [B, 128, H, W], x [B, 256, H, W], weights / biases in the order convz1, convr1, convq1, convz2, convr2, convq2 ->
    the new h, f64.  details: also the list per half of (z, r, q)."""
    h = np.asarray(h, np.float64)
    x = np.asarray(x, np.float64)
    kept = []
    for half, axis in ((0, 3), (1, 2)):
        wz, wr, wq = (np.asarray(weights[3 * half + i], np.float64).reshape(128, 384, 5) for i in range(3))
        bz, br, bq = (np.asarray(biases[3 * half + i], np.float64) for i in range(3))
        hx = np.concatenate([h, x], 1)
        z = _sigmoid(_conv(hx, wz, bz, axis))
        r = _sigmoid(_conv(hx, wr, br, axis))
        q = np.tanh(_conv(np.concatenate([r * h, x], 1), wq, bq, axis))
        h = (1.0 - z) * h + z * q
        kept.append((z, r, q))
    return (h, kept) if details else h


def bar(delta, scale):
    """The suite's bar of an f32 kernel against the f64 restatement: 8 x the reference's own f32 error for the case (never below
    one f32 ulp of the output scale)."""
    return 8.0 * max(float(delta), EPS32 * float(scale))


def load_reference():
    """SepConvGRU of the reference checkout (ROBUST_CVD_REFERENCE, default /root/reference), or None where it (or torch) is not
    available."""
    root = os.environ.get("ROBUST_CVD_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(root, "raft", "core", "update.py")):
        return None
    try:
        import torch  # noqa: F401
    except ImportError:
        return None
    added = root not in sys.path
    if added:
        sys.path.insert(0, root)
    try:
        from raft.core.update import SepConvGRU
    finally:
        if added:
            sys.path.remove(root)
    return SepConvGRU


def state_dict(case):
    """The case's parameters under the reference's names, as torch tensors."""
    import torch
    from tests.raftgru_cases import PARAMETERS
    sd = {}
    for n, w, b in zip(PARAMETERS, case["weights"], case["biases"]):
        sd[n + ".weight"], sd[n + ".bias"] = torch.from_numpy(w.copy()), torch.from_numpy(b.copy())
    return sd


def reference_output(SepConvGRU, case):
    """The reference module's f32 result on the CPU, [B, 128, H, W]."""
    import torch
    module = SepConvGRU(hidden_dim=128, input_dim=256)
    module.load_state_dict(state_dict(case))
    with torch.no_grad():
        return module(torch.from_numpy(case["h"]), torch.from_numpy(case["x"])).numpy()
