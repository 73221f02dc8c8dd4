"""Mints midas_golden.npz on the CPU from the reference's own classes (monodepth/midas_v2/blocks.py Interpolate, ResidualConvUnit,
FeatureFusionBlock; midas_net.py MidasNet; the checkout named by ROBUST_CVD_REFERENCE), never from the project's kernels:

    python -m tests.golden.reference_py.make_midas_golden

Per seeded case of tests/midas_cases.py: the reference's f32 output at the case's sampled pixels, delta = max |reference f32 -
float64 restatement| over ALL pixels, scale = max |restatement|, and the digest of the inputs (the inputs are not stored).  Single
convolutions run through nn.Conv2d and torch's relu and sums in the kernel's stated epilogue order, upsamplings through
nn.functional.interpolate and the reference's Interpolate, the head through the reference network's own output_conv[2:], the unit
and fusion-block cases through the reference's ResidualConvUnit and FeatureFusionBlock (on copies: they rectify their inputs in
place), whole decoders through the reference's MidasNet.forward over the case's stub backbone.

blocks.py imports iopath and torchvision at module level: stub modules stand in for exactly those names.  MidasNet.__init__ as
written calls torch.hub.load: midas_net._make_encoder is replaced by a function that returns the stub backbone and the reference's
own _make_scratch, and torch.hub.load by a function that raises (tests/midas_reference.py: load_reference, reference_net).  Also the
reference network's `scratch.*` state-dict keys."""
import numpy as np
import torch

from tests import midas_cases as mc
from tests import midas_reference as mr


def store(out, key, case, ref, want, samples):
    out[f"{key}/out"] = mc.sample_view(ref, samples)
    out[f"{key}/out_delta"] = np.float64(np.abs(ref.astype(np.float64) - want).max())
    out[f"{key}/out_scale"] = np.float64(np.abs(want).max())
    out[f"{key}/input_sha256"] = np.frombuffer(mc.input_digest(case).encode(), np.uint8)


def t(a):
    return torch.from_numpy(np.array(a))


def reference_conv(case):
    w = case["weight"]
    conv = torch.nn.Conv2d(w.shape[1], w.shape[0], case["k"], padding=case["k"] // 2, bias=case["bias"] is not None)
    conv.load_state_dict({"weight": t(w)} if case["bias"] is None else {"weight": t(w), "bias": t(case["bias"])})
    x = t(case["x"])
    y = conv(torch.relu(x) if case["relu_in"] else x)
    if case["relu"]:
        y = torch.relu(y)
    if case["a"] is not None:
        y = y + (torch.relu(t(case["a"])) if case["relu_a"] else t(case["a"]))
    if case["b"] is not None:
        y = t(case["b"]) + y
    return y.numpy()


def load_unit(unit, weights, biases):
    unit.load_state_dict({"conv1.weight": t(weights[0]), "conv1.bias": t(biases[0]), "conv2.weight": t(weights[1]), "conv2.bias": t(biases[1])},
                         strict=True)
    return unit


def main():
    reference = mr.load_reference()
    assert reference is not None, "the reference checkout is not available"
    blocks, _midas_net = reference
    out = {}
    with torch.no_grad():
        for name in mc.CONV_CASES:
            case = mc.make_conv_case(name)
            store(out, "conv/" + name, case, reference_conv(case), mr.conv_case(case), case["samples"])
        for name in mc.UPSAMPLE_CASES:
            case = mc.make_upsample_case(name)
            if case["align_corners"]:
                ref = torch.nn.functional.interpolate(t(case["x"]), scale_factor=2, mode="bilinear", align_corners=True)
            else:
                ref = blocks.Interpolate(scale_factor=2, mode="bilinear")(t(case["x"]))
            store(out, "upsample/" + name, case, ref.numpy(), mr.upsample2x(case["x"], case["align_corners"]), case["samples"])
        for name in mc.UNIT_CASES:
            case = mc.make_unit_case(name)
            unit = load_unit(blocks.ResidualConvUnit(case["x"].shape[1]), case["weights"], case["biases"]).eval()
            store(out, "unit/" + name, case, unit(t(case["x"])).numpy(), mr.unit_case(case), case["samples"])
        for name in mc.FUSION_CASES:
            case = mc.make_fusion_case(name)
            block = blocks.FeatureFusionBlock(case["x0"].shape[1]).eval()
            load_unit(block.resConfUnit1, case["weights"][0:2], case["biases"][0:2])
            load_unit(block.resConfUnit2, case["weights"][2:4], case["biases"][2:4])
            store(out, "fusion/" + name, case, block(t(case["x0"]), t(case["x1"])).numpy(), mr.fusion_case(case), case["samples"])
        keys = None
        nets = {}
        for name in mc.DECODER_CASES:
            case = mc.make_decoder_case(name)
            net = mr.reference_net(reference, case)
            nets[case["non_negative"]] = net
            keys = [k for k in net.state_dict().keys() if k.startswith("scratch.")]
            assert tuple(keys) == mc.STATE_DICT_KEYS and len(keys) == 42
            maps = [t(m) for m in case["maps"]]
            x = t(case["images"])
            for k in range(4):      # the stub backbone's features are exact: the cases test the decoder alone
                x = getattr(net.pretrained, f"layer{k + 1}")(x)
                assert torch.equal(x, maps[k]), (name, k)
            ref = net(t(case["images"])).numpy()
            store(out, "decoder/" + name, case, ref, mr.decoder_case(case), case["samples"])
            print(name, float(out[f"decoder/{name}/out_delta"]), float(out[f"decoder/{name}/out_scale"]), float((ref == 0).mean()))
        for name in mc.HEAD_CASES:
            case = mc.make_head_case(name)
            tail = nets[case["non_negative"]].scratch.output_conv[2:]
            tail.load_state_dict({"2.weight": t(case["weight2"]), "2.bias": t(case["bias2"]), "4.weight": t(case["weight4"]),
                                  "4.bias": t(case["bias4"])}, strict=True)
            ref = tail(t(case["x"]))[:, 0].numpy()
            store(out, "head/" + name, case, ref, mr.head_case(case), case["samples"])
            print(name, "negative share before the last ReLU", float((mr.head(case["x"], case["weight2"], case["bias2"], case["weight4"],
                                                                               case["bias4"], False) < 0).mean()))
    for key in sorted(k for k in out if k.endswith("out_delta")):
        print(key, float(out[key]), float(out[key.replace("out_delta", "out_scale")]))
    out["state_dict_keys"] = np.array(keys)
    np.savez_compressed(mr.GOLDEN, **out)


if __name__ == "__main__":
    main()
