"""Mints raftenc_golden.npz on the CPU from the reference's own modules (raft/core/extractor.py ResidualBlock / BasicEncoder,
raft/core/raft.py RAFT; the checkout named by ROBUST_CVD_REFERENCE), never from the project's kernels:

    python -m tests.golden.reference_py.make_raftenc_golden

Per seeded case of tests/raftenc_cases.py: the reference's f32 output at the case's sampled pixels, delta = max |reference f32 -
float64 restatement| over ALL pixels, scale = max |restatement|, and the digest of the inputs (the inputs are not stored).  Single
convolutions and instance norms run through the reference's layers' own functions (nn.Conv2d, nn.BatchNorm2d in eval mode,
nn.InstanceNorm2d, ReLU, the residual sum of ResidualBlock.forward); whole encoders through BasicEncoder; the two RAFT cases through
RAFT(test_mode=True), their restatement being tests/raftenc_reference.py's stock_raft in f64.  Also the reference RAFT's state-dict
keys."""
import argparse

import numpy as np
import torch

from tests import raftenc_cases as ec
from tests import raftenc_reference as er


def digest(case):
    return np.frombuffer(ec.input_digest(case).encode(), np.uint8)


def store(out, key, case, ref, want, samples):
    out[f"{key}/out"] = ec.sample_view(ref, samples)
    out[f"{key}/out_delta"] = np.float64(np.abs(ref.astype(np.float64) - want).max())
    out[f"{key}/out_scale"] = np.float64(np.abs(want).max())
    out[f"{key}/input_sha256"] = digest(case)


def reference_conv(case):
    w = case["weight"]
    conv = torch.nn.Conv2d(w.shape[1], w.shape[0], case["k"], stride=case["stride"], padding=case["k"] // 2)
    conv.load_state_dict({"weight": torch.from_numpy(w), "bias": torch.from_numpy(case["bias"])})
    y = conv(torch.from_numpy(case["x"]))
    if case["norm"] is not None:
        norm = torch.nn.BatchNorm2d(w.shape[0]).eval()
        norm.load_state_dict(dict(zip(ec.NORM_VECTORS, map(torch.from_numpy, case["norm"]))), strict=False)
        y = norm(y)
    if case["relu"]:
        y = torch.relu(y)
    if case["residual"] is not None:
        y = torch.relu(torch.from_numpy(case["residual"]) + y)
    return y.numpy()


def reference_norm(case):
    y = torch.nn.InstanceNorm2d(case["x"].shape[1])(torch.from_numpy(case["x"]))
    if case["relu"]:
        y = torch.relu(y)
    if case["residual"] is not None:
        y = torch.relu(torch.from_numpy(case["residual"]) + y)
    return y.numpy()


def main():
    BasicEncoder, RAFT = er.load_reference()
    out = {}
    with torch.no_grad():
        for name in ec.CONV_CASES:
            case = ec.make_conv_case(name)
            store(out, "conv/" + name, case, reference_conv(case), er.conv_case(case), case["samples"])
        for name in ec.NORM_CASES:
            case = ec.make_norm_case(name)
            store(out, "norm/" + name, case, reference_norm(case), er.norm_case(case), case["samples"])
        for name in ec.ENCODER_CASES:
            case = ec.make_encoder_case(name)
            module = BasicEncoder(output_dim=ec.OUTPUT_DIM, norm_fn=case["norm_mode"], dropout=0.0).eval()
            module.load_state_dict(er.encoder_state_dict(case), strict=True)
            store(out, "encoder/" + name, case, module(torch.from_numpy(case["images"])).numpy(), er.encoder_case(case), case["samples"])
            print(name, float(out[f"encoder/{name}/out_delta"]), float(out[f"encoder/{name}/out_scale"]))
        keys = None
        for name in ec.RAFT_CASES:
            case = ec.make_raft_case(name)
            module = RAFT(argparse.Namespace(small=False, mixed_precision=False)).eval()
            keys = list(module.state_dict().keys())
            module.load_state_dict(er.raft_state_dict(case), strict=True)
            i1, i2 = torch.from_numpy(case["image1"]), torch.from_numpy(case["image2"])
            low, up = module(i1, i2, iters=case["iters"], test_mode=True)
            low64, up64 = er.stock_raft(er.raft_state_dict(case), i1, i2, case["iters"], torch.float64)
            for o, ref, want, samples in (("flow_low", low, low64, case["samples_low"]), ("flow_up", up, up64, case["samples_up"])):
                out[f"raft/{name}/{o}"] = ec.sample_view(ref.numpy(), samples)
                out[f"raft/{name}/{o}_delta"] = np.float64((ref.double() - want).abs().max())
                out[f"raft/{name}/{o}_scale"] = np.float64(want.abs().max())
                print(name, o, float(out[f"raft/{name}/{o}_delta"]), float(out[f"raft/{name}/{o}_scale"]))
            out[f"raft/{name}/input_sha256"] = digest(case)
    out["state_dict_keys"] = np.array(keys)
    np.savez_compressed(er.GOLDEN, **out)


if __name__ == "__main__":
    main()
