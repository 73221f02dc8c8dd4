"""float64 numpy restatement of the convolutions of the reference's update block and of BasicUpdateBlock.forward
(raft/core/update.py:8-16, 96-114, 133-156) for robust_cvd_amd/csrc/cvd_raftconv.h, and the bar of the GPU tests.  The mathematics
in double, from the f32 inputs, as im2col + matmul; the GRU in the middle is tests/raftgru_reference.py's.  The fixture
(raftblock_golden.npz, minted by tests/golden/reference_py/make_raftblock_golden.py) records how far the reference's own f32
arithmetic is from it."""
import os
import sys

import numpy as np

from tests import raftgru_reference as gr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_py", "raftblock_golden.npz")
EPS32 = 2.0 ** -23


def conv2d(x, weight, bias, relu=False, scale=1.0):
    """x [B, C, H, W]; weight [O, C, k, k], stride 1, zero padding k // 2; -> scale * act(conv + bias), [B, O, H, W] f64."""
    x = np.asarray(x, np.float64)
    weight = np.asarray(weight, np.float64)
    B, C, H, W = x.shape
    O, C2, k, k2 = weight.shape
    assert C == C2 and k == k2 and k % 2 == 1
    r = k // 2
    padded = np.pad(x, ((0, 0), (0, 0), (r, r), (r, r)))
    # im2col: columns[b, (c k + i) k + j, y, x] = padded[b, c, y + i, x + j]
    columns = np.empty((B, C, k, k, H, W), np.float64)
    for i in range(k):
        for j in range(k):
            columns[:, :, i, j] = padded[:, :, i:i + H, j:j + W]
    out = np.matmul(weight.reshape(O, C * k * k), columns.reshape(B, C * k * k, H * W)).reshape(B, O, H, W)
    out += np.asarray(bias, np.float64).reshape(1, O, 1, 1)
    if relu:
        out = np.maximum(out, 0.0)
    return scale * out


def conv_case(case):
    """The single-convolution case's output, [B, N, H, W] f64 (stacked weights along the channels)."""
    return np.concatenate([conv2d(case["x"], w, b, case["relu"], case["scale"]) for w, b in zip(case["weights"], case["biases"])], 1)


def update_block(net, inp, corr, flow, weights, biases, details=False):
    """-> (net, mask, delta_flow) f64; details: also the dict of the intermediates by name."""
    w = [np.asarray(a, np.float64) for a in weights]
    b = [np.asarray(a, np.float64) for a in biases]
    flow64 = np.asarray(flow, np.float64)
    cor1 = conv2d(corr, w[0], b[0], True)
    cor2 = conv2d(cor1, w[1], b[1], True)
    flo1 = conv2d(flow64, w[2], b[2], True)
    flo2 = conv2d(flo1, w[3], b[3], True)
    cor_flo = np.concatenate([cor2, flo2], 1)
    motion = np.concatenate([conv2d(cor_flo, w[4], b[4], True), flow64], 1)
    x = np.concatenate([np.asarray(inp, np.float64), motion], 1)
    new_net = gr.sepconv_gru(net, x, w[5:11], b[5:11])
    flow_hidden = conv2d(new_net, w[11], b[11], True)
    delta_flow = conv2d(flow_hidden, w[12], b[12])
    mask_hidden = conv2d(new_net, w[13], b[13], True)
    mask = conv2d(mask_hidden, w[14], b[14], False, 0.25)
    if details:
        return new_net, mask, delta_flow, {"cor1": cor1, "cor_flo": cor_flo, "flo1": flo1, "motion_features": motion,
                                           "flow_hidden": flow_hidden, "mask_hidden": mask_hidden}
    return new_net, mask, delta_flow


def block_case(case, details=False):
    return update_block(case["net"], case["inp"], case["corr"], case["flow"], case["weights"], case["biases"], details)


def bar(delta, scale):
    """The project's f32 bar against the f64 restatement: 8 x the reference's own f32 error for the case (never below one f32 ulp
    of the output scale)."""
    return 8.0 * max(float(delta), EPS32 * float(scale))


def load_reference():
    """BasicUpdateBlock of the reference checkout (ROBUST_CVD_REFERENCE, default /root/reference), or None where it (or torch) is
    not available."""
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
        from raft.core.update import BasicUpdateBlock
    finally:
        if added:
            sys.path.remove(root)
    return BasicUpdateBlock


class Args:
    """What the reference's BasicMotionEncoder reads of RAFT's arguments."""
    corr_levels = 4
    corr_radius = 4


def state_dict(case):
    """The block case's parameters under the reference's names, as torch tensors."""
    import torch
    from tests.raftblock_cases import PARAMETERS
    sd = {}
    for n, w, b in zip(PARAMETERS, case["weights"], case["biases"]):
        sd[n + ".weight"], sd[n + ".bias"] = torch.from_numpy(w.copy()), torch.from_numpy(b.copy())
    return sd


def reference_block_output(BasicUpdateBlock, case):
    """The reference module's f32 results on the CPU: (net, mask, delta_flow)."""
    import torch
    module = BasicUpdateBlock(Args(), hidden_dim=128, input_dim=128)
    module.load_state_dict(state_dict(case))
    with torch.no_grad():
        out = module(*(torch.from_numpy(case[k]) for k in ("net", "inp", "corr", "flow")))
    return tuple(t.numpy() for t in out)


def reference_conv_output(case):
    """The single-convolution case as the reference's layers compute it on the CPU in f32: nn.Conv2d's function, F.relu, the
    factor (raft/core/update.py:16, 107-113, 155)."""
    import torch
    import torch.nn.functional as F
    outs = []
    with torch.no_grad():
        for w, b in zip(case["weights"], case["biases"]):
            y = F.conv2d(torch.from_numpy(case["x"]), torch.from_numpy(w), torch.from_numpy(b), padding=case["k"] // 2)
            if case["relu"]:
                y = F.relu(y)
            if case["scale"] != 1.0:
                y = case["scale"] * y
            outs.append(y)
    return torch.cat(outs, 1).numpy()
