"""Child process of tests/test_gpu_midas.py::test_torch_modules (python -m tests.midas_torch_child): torch is imported first, then the
library; robust_cvd_amd.midas.MidasNet over the cases' stub backbone on GPU tensors against the array path (Solver.midas_decoder),
the float64 restatement and the reference's stored values, with the bars of tests/test_gpu_midas.py; ResidualConvUnit,
FeatureFusionBlock and Interpolate against the stored values of the reference's own classes; the state-dict load as the reference
saves and loads it; a run on a side stream with torch's synchronisation check armed; estimate_depth; the refusals."""
import io

import numpy as np
import torch

from robust_cvd_amd import midas
from robust_cvd_amd import torch_common as tc
from tests import margins
from tests import midas_cases as mc
from tests import midas_reference as mr

DEV = torch.device("cuda", 0)


def raises(exc, call, word=None):
    try:
        call()
    except exc as e:
        assert word is None or word in str(e), (word, str(e))
    else:
        raise AssertionError(f"{exc.__name__} expected")


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def net_of(case):
    net = midas.MidasNet(features=case["features"], non_negative=case["non_negative"], backbone=mr.stub_backbone(case["stub"]))
    assert tuple(k for k in net.state_dict() if k.startswith("scratch.")) == mc.STATE_DICT_KEYS
    sd = net.state_dict()
    sd.update(mr.scratch_state_dict(case))
    result = net.load_state_dict(sd, strict=True)                     # the reference's names and shapes
    assert not result.missing_keys and not result.unexpected_keys
    return net.to(DEV).eval()


def within(label, golden, key, case, got, want):
    delta = float(golden[f"{key}/out_delta"])
    bar = mr.bar(delta, golden[f"{key}/out_scale"])
    assert got.shape == want.shape and got.dtype == np.float32
    margins.below(label, np.abs(got - want).max(), bar)
    margins.below(f"{label} vs reference", np.abs(mc.sample_view(got, case["samples"]) - golden[f"{key}/out"]).max(), bar + delta)


def check_net(solver, golden, name):
    case = mc.make_decoder_case(name)
    net = net_of(case)
    images = gpu(case["images"])
    with torch.no_grad():
        maps, x = [], images
        for k in range(4):            # the stub backbone is exact on the GPU too
            x = getattr(net.pretrained, f"layer{k + 1}")(x)
            maps.append(x)
            assert np.array_equal(x.cpu().numpy(), case["maps"][k]), (name, k)
        kept = [m.clone() for m in maps]
        out = net(images)
        assert all(torch.equal(a, b) for a, b in zip(kept, maps))     # the caller's feature maps are as they were
        assert torch.equal(net.decode(*maps), out)
    got = out.cpu().numpy()
    assert out.is_contiguous() and tuple(out.shape) == (images.shape[0],) + tuple(images.shape[2:])
    assert np.array_equal(got, solver.midas_decoder(case["maps"], case["weights"], case["biases"], non_negative=case["non_negative"])), name
    within(f"midas net torch {name}", golden, "decoder/" + name, case, got, mr.decoder_case(case))
    return net, images, out


def check_blocks(golden):
    case = mc.make_unit_case("rcu_64_6x7")
    unit = midas.ResidualConvUnit(64)
    unit.load_state_dict({"conv1.weight": torch.from_numpy(case["weights"][0]), "conv1.bias": torch.from_numpy(case["biases"][0]),
                          "conv2.weight": torch.from_numpy(case["weights"][1]), "conv2.bias": torch.from_numpy(case["biases"][1])}, strict=True)
    unit = unit.to(DEV).eval()
    x = gpu(case["x"])
    with torch.no_grad():
        got = unit(x)
    assert np.array_equal(x.cpu().numpy(), case["x"])                  # not rectified in place: the caller's tensor is as it was
    within("midas unit torch", golden, "unit/rcu_64_6x7", case, got.cpu().numpy(), mr.unit_case(case))
    case = mc.make_fusion_case("ffb_64_5x6b2")
    block = midas.FeatureFusionBlock(64)
    names = [f"resConfUnit{u}.conv{c}" for u in (1, 2) for c in (1, 2)]
    sd = {}
    for n, w, b in zip(names, case["weights"], case["biases"]):
        sd[n + ".weight"], sd[n + ".bias"] = torch.from_numpy(w), torch.from_numpy(b)
    block.load_state_dict(sd, strict=True)
    block = block.to(DEV).eval()
    x0, x1 = gpu(case["x0"]), gpu(case["x1"])
    with torch.no_grad():
        got = block(x0, x1)
        one = block(x0)
    assert np.array_equal(x0.cpu().numpy(), case["x0"]) and np.array_equal(x1.cpu().numpy(), case["x1"])
    within("midas fusion block torch", golden, "fusion/ffb_64_5x6b2", case, got.cpu().numpy(), mr.fusion_case(case))
    want = mr.feature_fusion_block([case["x0"]], case["weights"], case["biases"])
    assert np.abs(one.cpu().numpy() - want).max() <= mr.bar(golden["fusion/ffb_64_5x6b2/out_delta"], golden["fusion/ffb_64_5x6b2/out_scale"])
    case = mc.make_upsample_case("half_3x5")
    with torch.no_grad():
        got = midas.Interpolate(scale_factor=2, mode="bilinear")(gpu(case["x"]))
    within("midas interpolate torch", golden, "upsample/half_3x5", case, got.cpu().numpy(), mr.upsample2x(case["x"], False))
    raises(ValueError, lambda: midas.Interpolate(scale_factor=4, mode="bilinear"), "scale_factor 2")


def check_data_parallel_load(name):
    """As the reference saves and loads a checkpoint: saved from a DataParallel wrapper, loaded into one, used through .module."""
    case = mc.make_decoder_case(name)
    net = midas.MidasNet(features=case["features"], backbone=mr.stub_backbone(case["stub"]))
    sd = net.state_dict()
    sd.update(mr.scratch_state_dict(case))
    buf = io.BytesIO()
    torch.save({"module." + k: v for k, v in sd.items()}, buf)
    buf.seek(0)
    wrapped = torch.nn.DataParallel(midas.MidasNet(features=case["features"], backbone=mr.stub_backbone(case["stub"])))
    result = wrapped.load_state_dict(torch.load(buf), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    # (with one visible device the wrapper moves its module there)
    assert torch.equal(wrapped.module.scratch.output_conv[4].bias.cpu(), sd["scratch.output_conv.4.bias"])
    assert torch.equal(wrapped.module.scratch.refinenet4.resConfUnit1.conv1.weight.cpu(), sd["scratch.refinenet4.resConfUnit1.conv1.weight"])


def check_no_host_synchronisation(net, images, out):
    """Once the handle's scratch has its size a call is enqueued launches only: torch's synchronisation check stays silent, also on
    a side stream."""
    torch.cuda.synchronize(DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            again = net(images)
            side = torch.cuda.Stream(device=DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                third = net(images)
            torch.cuda.current_stream(DEV).wait_stream(side)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize(DEV)
    assert torch.equal(again, out) and torch.equal(third, out)


def check_estimate_depth(net):
    rng = np.random.default_rng(11)
    images = gpu(rng.uniform(0.0, 1.0, (2, 1, 3, 64, 64)).astype(np.float32))
    with torch.no_grad():
        depth = midas.estimate_depth(net, images)
        # the six lines of MidasV2Model.estimate_depth
        shape = images.shape
        input_ = images.reshape(-1, 3, 64, 64)
        input_ = (input_ - torch.Tensor([0.485, 0.456, 0.406]).reshape(1, -1, 1, 1).to(DEV)) / torch.Tensor([0.229, 0.224, 0.225]).reshape(1, -1, 1, 1).to(DEV)
        output = net(input_)
        disparity = output.reshape(shape[:-3] + output.shape[-2:])
        want = (0.0000001 + disparity).reciprocal()
    assert depth.shape == (2, 1, 64, 64) and torch.equal(depth, want) and torch.isfinite(depth).all()


def check_refusals(net, images):
    with torch.no_grad():
        raises(ValueError, lambda: net(images.cpu()), "GPU")
        raises(TypeError, lambda: net(images.double()), "float32")
        raises(ValueError, lambda: net(images[:, :, :-4]), "multiples of 32")
        raises(ValueError, lambda: net(images[0]), "(B, C, H, W)")
        fresh = midas.MidasNet(features=64, backbone=net.pretrained)
        raises(ValueError, lambda: fresh.to(DEV)(images), "training mode")            # a fresh module is in training mode
        maps = [torch.zeros(1, c, 8 >> k, 8 >> k, device=DEV) for k, c in enumerate(mc.BACKBONE_CHANNELS)]
        raises(ValueError, lambda: net.decode(maps[0], maps[1], maps[2], maps[3][:, :, :, :0]), "= 0")
        raises(ValueError, lambda: net.decode(maps[0], maps[1], maps[1], maps[3]), "feature map")
        raises(ValueError, lambda: net.decode(maps[0], maps[1].cpu(), maps[2], maps[3]), "GPU")
        raises(TypeError, lambda: net.decode(maps[0], maps[1].half(), maps[2], maps[3]), "float32")
        unit = net.scratch.refinenet1.resConfUnit2
        x = torch.zeros(1, unit.conv1.weight.shape[1], 4, 4, device=DEV)
        raises(ValueError, lambda: unit(x.cpu()), "GPU")
        raises(ValueError, lambda: unit(x[:, :8]), "channels")
        raises(ValueError, lambda: net.scratch.refinenet1(x, x[:, :, :2]), "one shape")
        raises(ValueError, lambda: net.scratch.refinenet1(x, x, x), "one or two")
        cpu_net = midas.MidasNet(features=64, backbone=mr.stub_backbone(mc.make_stub(np.random.default_rng(3)))).eval()
        raises(ValueError, lambda: cpu_net(images), "different devices")               # parameters on the CPU
    # grad mode on: the parameters require grad
    raises(RuntimeError, lambda: net(images), "forward only")
    for p in net.parameters():
        p.requires_grad_(False)
    raises(RuntimeError, lambda: net(images.clone().requires_grad_(True)), "forward only")
    torch.cuda.synchronize(DEV)
    assert net(images).shape == (images.shape[0],) + tuple(images.shape[2:])
    if torch.cuda.device_count() > 1:
        raises(ValueError, lambda: net.decode(*[m.to("cuda:1") if k == 2 else m for k, m in enumerate(
            [torch.zeros(1, c, 8 >> k, 8 >> k, device=DEV) for k, c in enumerate(mc.BACKBONE_CHANNELS)])]), "different devices")
    torch.cuda.synchronize(DEV)


if __name__ == "__main__":
    torch.cuda.init()
    golden = np.load(mr.GOLDEN)
    solver = tc.solver(DEV)
    kept = None
    for name in ("f256_64x96", "f256_96x64b2", "f64_64x64"):
        kept = check_net(solver, golden, name)
    check_blocks(golden)
    check_data_parallel_load("f64_64x64")
    check_no_host_synchronisation(*kept)
    check_estimate_depth(kept[0])
    check_refusals(kept[0], kept[1])
    print("midas torch modules ok")
