"""Mints resnext_golden.npz on the CPU from STOCK TORCH f32 modules wired as torchvision's Bottleneck / ResNet
(tests/resnext_reference.py: stock_resnet), never from the project's kernels:

    python -m tests.golden.reference_py.make_resnext_golden

torchvision is not needed: the reference builds its backbone from it through torch.hub, which nothing here may call.  Where
torchvision is importable the script also builds ResNet(Bottleneck, ...) itself and asserts the same key list, shapes and output bit
for bit.  Per seeded case of tests/resnext_cases.py: torch's f32 output at the case's sampled pixels, delta = max |torch f32 -
float64 restatement| over ALL pixels, scale = max |restatement|, and the digest of the inputs (the inputs are not stored).  Single
convolutions run through nn.Conv2d(groups=...), nn.BatchNorm2d in eval mode, torch.relu and the residual sum; the pool through
nn.MaxPool2d(3, 2, 1); bottlenecks and backbones through the stock modules; the whole network through the REFERENCE's own
midas_net.MidasNet.forward (the checkout named by ROBUST_CVD_REFERENCE), whose _make_encoder is replaced by the stock backbone plus
the reference's own _make_scratch, as make_midas_golden.py does with its stub.  The conditions on the inputs (finite maps, 10 % to
90 % zeros, a scale within [1e-3, 1e3]) are asserted for every backbone case."""
import numpy as np
import torch

from tests import midas_reference as mr
from tests import resnext_cases as rc
from tests import resnext_reference as rr


def store(out, key, case, ref, want, samples):
    out[f"{key}/out"] = rc.sample_view(ref, samples)
    out[f"{key}/out_delta"] = np.float64(np.abs(ref.astype(np.float64) - want).max())
    out[f"{key}/out_scale"] = np.float64(np.abs(want).max())
    out[f"{key}/input_sha256"] = np.frombuffer(rc.input_digest(case).encode(), np.uint8)


def t(a):
    return torch.from_numpy(np.array(a))


def batch_norm(n, four):
    bn = torch.nn.BatchNorm2d(n, eps=rc.EPS)
    bn.load_state_dict({"weight": t(four[0]), "bias": t(four[1]), "running_mean": t(four[2]), "running_var": t(four[3]),
                        "num_batches_tracked": torch.tensor(0)})
    return bn.eval()


def reference_conv(case, groups=1):
    w = case["weight"]
    k = w.shape[2]
    conv = torch.nn.Conv2d(w.shape[1] * groups, w.shape[0], k, stride=case["stride"], padding=k // 2, groups=groups, bias=False)
    conv.load_state_dict({"weight": t(w)})
    y = conv(t(case["x"]))
    if case["norm"] is not None:
        y = batch_norm(w.shape[0], case["norm"])(y)
    if case["relu"]:
        y = torch.relu(y)
    if case.get("residual") is not None:
        y = torch.relu(t(case["residual"]) + y)
    return y.numpy()


def reference_block(case):
    inplanes, planes, stride, groups, wpg, _shape = rc.BLOCK_CASES[case["name"]]
    # one stage of the stock ResNet holds exactly this block: build the smallest network that has it and take the block out
    resnet = rr.stock_resnet((1, 1, 1, 1), groups, wpg)
    stage = {64: 1, 128: 2, 256: 3, 512: 4}[planes]
    block = getattr(resnet, f"layer{stage}")[0]
    names = ["conv1", "conv2", "conv3", "downsample.0"]
    norms = ["bn1", "bn2", "bn3", "downsample.1"]
    if len(case["params"]) == 3:                       # no downsample: the block as a stage's later blocks have it
        resnet = rr.stock_resnet((2, 2, 2, 2), groups, wpg)
        block = getattr(resnet, f"layer{stage}")[1]
    sd = {}
    for name, norm, (w, four) in zip(names, norms, case["params"]):
        sd[name + ".weight"] = t(w)
        for v, a in zip(rc.NORM_KEYS, four):
            sd[f"{norm}.{v}"] = t(a)
        sd[f"{norm}.num_batches_tracked"] = torch.tensor(0)
    block.load_state_dict(sd, strict=True)
    assert block.conv2.stride == (stride, stride) and block.conv1.in_channels == inplanes
    return block.eval()(t(case["x"])).numpy()


def check_against_torchvision(case, maps):
    """Where torchvision is importable: its own ResNet(Bottleneck, ...) has the same keys and shapes and gives the same maps."""
    try:
        from torchvision.models.resnet import Bottleneck, ResNet
    except ImportError:
        return False
    tv = ResNet(Bottleneck, list(case["blocks"]), groups=case["groups"], width_per_group=case["width_per_group"])
    mine = rr.stock_resnet(case["blocks"], case["groups"], case["width_per_group"])
    theirs = {k: tuple(v.shape) for k, v in tv.state_dict().items() if not k.startswith("fc.")}
    assert list(theirs.items()) == [(k, tuple(v.shape)) for k, v in mine.state_dict().items()]
    rr.load_parameters(mine, case["params"], case["blocks"], case["groups"], case["width_per_group"])
    sd = dict(mine.state_dict(), **{"fc.weight": tv.fc.weight, "fc.bias": tv.fc.bias})
    tv.load_state_dict(sd, strict=True)
    for a, b in zip(rr.stock_maps(rr.midas_backbone(tv).eval(), case["images"]), maps):
        assert torch.equal(a, b)
    return True


def main():
    reference = mr.load_reference()
    assert reference is not None, "the reference checkout is not available"
    out = {}
    with torch.no_grad():
        for name in rc.GROUPED_CASES:
            case = rc.make_grouped_case(name)
            store(out, "grouped/" + name, case, reference_conv(case, case["groups"]), rr.grouped_case(case), case["samples"])
        for name in rc.CONV_CASES:
            case = rc.make_conv_case(name)
            store(out, "conv/" + name, case, reference_conv(case), rr.conv_case(case), case["samples"])
        for name in rc.POOL_CASES:
            case = rc.make_pool_case(name)
            store(out, "pool/" + name, case, torch.nn.MaxPool2d(3, 2, 1)(t(case["x"])).numpy(), rr.maxpool(case["x"]), case["samples"])
        for name in rc.BLOCK_CASES:
            case = rc.make_block_case(name)
            store(out, "block/" + name, case, reference_block(case), rr.block_case(case), case["samples"])
        for name in rc.BACKBONE_CASES:
            case = rc.make_backbone_case(name)
            pretrained = rr.stock_backbone(case)
            keys = [(k, tuple(v.shape)) for k, v in pretrained.state_dict().items()]
            assert [("pretrained." + k, s) for k, s in keys] == rc.state_dict_keys(case["blocks"], case["groups"], case["width_per_group"])
            maps = rr.stock_maps(pretrained, case["images"])
            want = rr.backbone_case(case)
            rr.check_conditions(name, want)
            rr.check_conditions(name, [m.numpy() for m in maps])
            print(name, "torchvision's own classes agree" if check_against_torchvision(case, maps) else "torchvision is not installed")
            for k in range(4):
                store(out, f"backbone/{name}/map{k + 1}", case, maps[k].numpy(), want[k], case["samples"][k])
                print(name, k + 1, "zeros", float((want[k] == 0).mean()), "scale", float(np.abs(want[k]).max()),
                      "delta", float(out[f"backbone/{name}/map{k + 1}/out_delta"]))
        for name in rc.NET_CASES:
            case = rc.make_net_case(name)
            net = rr.reference_net(reference, case)
            keys = list(net.state_dict().keys())
            assert keys == [k for k, _ in rc.state_dict_keys(case["blocks"], case["groups"], case["width_per_group"])] + list(rc.mc.STATE_DICT_KEYS)
            rr.check_conditions(name, rr.backbone_case(case))
            ref = net(t(case["images"])).numpy()
            store(out, "net/" + name, case, ref, rr.net_case(case), case["samples"])
            print(name, float(out[f"net/{name}/out_delta"]), float(out[f"net/{name}/out_scale"]), float((ref == 0).mean()))
    for key in sorted(k for k in out if k.endswith("out_delta")):
        print(key, float(out[key]), float(out[key.replace("out_delta", "out_scale")]))
    np.savez_compressed(rr.GOLDEN, **out)


if __name__ == "__main__":
    main()
