"""Child process of tests/test_gpu_resnext.py::test_torch_modules (python -m tests.resnext_torch_child): torch is imported first, then
the library; robust_cvd_amd.midas's Bottleneck and ResNeXt on GPU tensors against the array path (Solver.midas_backbone), the float64
restatement and stock torch's stored values, with the bars of tests/test_gpu_resnext.py; the whole MidasNet with the native backbone
against the stored output of the reference's own MidasNet.forward; the state-dict keys and the strict load; the inputs left as they
were; a run with torch's synchronisation check armed; estimate_depth; the refusals."""
import numpy as np
import torch

from robust_cvd_amd import midas
from robust_cvd_amd import torch_common as tc
from tests import margins
from tests import midas_cases as mc
from tests import resnext_cases as rc
from tests import resnext_reference as rr

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


def within(label, golden, key, got, want, samples):
    delta = float(golden[f"{key}/out_delta"])
    bar = rr.bar(delta, golden[f"{key}/out_scale"])
    assert got.shape == want.shape and got.dtype == np.float32
    margins.below(label, np.abs(got - want).max(), bar)
    margins.below(f"{label} vs reference", np.abs(rc.sample_view(got, samples) - golden[f"{key}/out"]).max(), bar + delta)


def check_blocks(golden):
    for name in rc.BLOCK_CASES:
        case = rc.make_block_case(name)
        inplanes, planes, stride, groups, wpg, _shape = rc.BLOCK_CASES[name]
        down = None
        if len(case["params"]) == 4:
            down = torch.nn.Sequential(torch.nn.Conv2d(inplanes, 4 * planes, kernel_size=1, stride=stride, bias=False),
                                       torch.nn.BatchNorm2d(4 * planes))
        block = midas.Bottleneck(inplanes, planes, stride, down, groups, wpg)
        sd = {}
        for conv, norm, (w, four) in zip(("conv1", "conv2", "conv3", "downsample.0"), ("bn1", "bn2", "bn3", "downsample.1"), case["params"]):
            sd[conv + ".weight"] = torch.from_numpy(w)
            sd.update({f"{norm}.{v}": torch.from_numpy(a) for v, a in zip(rc.NORM_KEYS, four)})
            sd[f"{norm}.num_batches_tracked"] = torch.tensor(0)
        result = block.load_state_dict(sd, strict=True)
        assert not result.missing_keys and not result.unexpected_keys
        block = block.to(DEV).eval()
        x = gpu(case["x"])
        with torch.no_grad():
            got = block(x)
        assert np.array_equal(x.cpu().numpy(), case["x"])                     # the caller's tensor is as it was
        within(f"resnext bottleneck torch {name}", golden, "block/" + name, got.cpu().numpy(), rr.block_case(case), case["samples"])
        raises(ValueError, lambda: midas.Bottleneck(inplanes, planes, stride, None, groups, wpg).to(DEV)(x), "training mode")
        with torch.no_grad():
            raises(ValueError, lambda: block(x.cpu()), "GPU")
            raises(TypeError, lambda: block(x.double()), "float32")
            raises(ValueError, lambda: block(x[:, :8]), "channels")
        raises(RuntimeError, lambda: block(x), "forward only")                # grad mode on: the parameters require grad


def backbone_of(case):
    backbone = midas.ResNeXt(case["blocks"], case["groups"], case["width_per_group"])
    sd = {k[len("pretrained."):]: v for k, v in rr.pretrained_state_dict(case).items()}
    assert list(backbone.state_dict().keys()) == list(sd.keys())
    result = backbone.load_state_dict(sd, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    return backbone


def check_backbone(solver, golden, name):
    case = rc.make_backbone_case(name)
    backbone = backbone_of(case).to(DEV).eval()
    images = gpu(case["images"])
    kept = images.clone()
    with torch.no_grad():
        maps = backbone(images)
        staged, x = [], images
        for k in range(4):                      # the existing MidasNet.forward's way: layer1 .. layer4 as callables
            x = getattr(backbone, f"layer{k + 1}")(x)
            staged.append(x)
    assert torch.equal(images, kept)
    array = solver.midas_backbone(case["images"], [w for w, _ in case["params"]], [f for _, f in case["params"]], case["blocks"],
                                  case["groups"], case["width_per_group"], rc.EPS)
    want = rr.backbone_case(case)
    for k in range(4):
        got = maps[k].cpu().numpy()
        assert maps[k].is_contiguous() and torch.equal(staged[k], maps[k]), (name, k)      # ONE call == the stages' launches
        assert np.array_equal(got, array[k]), (name, k)
        within(f"resnext torch {name} map {k + 1}", golden, f"backbone/{name}/map{k + 1}", got, want[k], case["samples"][k])
    return backbone, images


def check_net(golden, name):
    case = rc.make_net_case(name)
    net = midas.MidasNet(features=case["features"], non_negative=case["non_negative"],
                         backbone=midas.ResNeXt(case["blocks"], case["groups"], case["width_per_group"]))
    want_keys = [k for k, _ in rc.state_dict_keys(case["blocks"], case["groups"], case["width_per_group"])] + list(mc.STATE_DICT_KEYS)
    assert list(net.state_dict().keys()) == want_keys
    sd = dict(rr.pretrained_state_dict(case), **rr.scratch_state_dict(case))
    assert list(sd.keys()) == want_keys
    result = net.load_state_dict(sd, strict=True)                             # the reference's names, order and shapes
    assert not result.missing_keys and not result.unexpected_keys
    net = net.to(DEV).eval()
    images = gpu(case["images"])
    kept = images.clone()
    with torch.no_grad():
        out = net(images)
        assert torch.equal(net.decode(*net.pretrained(images)), out)
        # the parent commit's form: the same backbone in stock torch ops inside MidasNet
        stock = midas.MidasNet(features=case["features"], non_negative=case["non_negative"], backbone=rr.stock_backbone(case))
        stock.load_state_dict(sd, strict=True)
        stock_out = stock.to(DEV).eval()(images)
    assert torch.equal(images, kept) and out.is_contiguous() and tuple(out.shape) == (1, 64, 64)
    got = out.cpu().numpy()
    want = rr.net_case(case)
    within(f"midas net native backbone {name}", golden, "net/" + name, got, want, case["samples"])
    delta = float(golden[f"net/{name}/out_delta"])
    margins.below(f"midas net {name}: native against the stock-torch backbone", np.abs(got - stock_out.cpu().numpy()).max(),
                  2 * rr.bar(delta, golden[f"net/{name}/out_scale"]))
    return net, images, out


def check_no_host_synchronisation(net, images, out):
    """Once the handle's scratch has its size a call is enqueued launches only: torch's synchronisation check stays silent."""
    torch.cuda.synchronize(DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            again = net(images)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize(DEV)
    assert torch.equal(again, out)


def check_estimate_depth(net):
    rng = np.random.default_rng(12)
    images = gpu(rng.uniform(0.0, 1.0, (2, 1, 3, 64, 64)).astype(np.float32))
    with torch.no_grad():
        depth = midas.estimate_depth(net, images)
        input_ = images.reshape(-1, 3, 64, 64)
        input_ = (input_ - torch.Tensor([0.485, 0.456, 0.406]).reshape(1, -1, 1, 1).to(DEV)) / torch.Tensor([0.229, 0.224, 0.225]).reshape(1, -1, 1, 1).to(DEV)
        want = (0.0000001 + net(input_).reshape(2, 1, 64, 64)).reciprocal()
    assert depth.shape == (2, 1, 64, 64) and torch.equal(depth, want)


def check_refusals(backbone, net, images):
    with torch.no_grad():
        raises(ValueError, lambda: backbone(images.cpu()), "GPU")
        raises(TypeError, lambda: backbone(images.double()), "float32")
        raises(ValueError, lambda: backbone(images[:, :, :-4]), "multiples of 32")
        raises(ValueError, lambda: backbone(images[:, :2]), "(B, 3, H, W)")
        raises(ValueError, lambda: backbone.layer1(images.cpu()), "GPU")
        raises(ValueError, lambda: net(images[:, :, :, :-4]), "multiples of 32")
        fresh = midas.ResNeXt(*rc.SMALL).to(DEV)
        raises(ValueError, lambda: fresh(images), "training mode")             # a fresh module is in training mode
        raises(ValueError, lambda: midas.ResNeXt(*rc.SMALL).eval()(images), "GPU")        # parameters on the CPU
        raises(ValueError, lambda: midas.ResNeXt((2, 1, 2, 1), 4, 12).to(DEV).eval()(images), "channels per group")
    raises(RuntimeError, lambda: backbone(images), "forward only")            # grad mode on: the parameters require grad
    for p in backbone.parameters():
        p.requires_grad_(False)
    raises(RuntimeError, lambda: backbone(images.clone().requires_grad_(True)), "forward only")
    assert len(backbone(images)) == 4
    torch.cuda.synchronize(DEV)
    assert midas.resnext101_32x8d().blocks == (3, 4, 23, 3)


if __name__ == "__main__":
    torch.cuda.init()
    golden = np.load(rr.GOLDEN)
    solver = tc.solver(DEV)
    check_blocks(golden)
    backbone, images = check_backbone(solver, golden, "small_64x96b2")
    check_backbone(solver, golden, "small_32x32")
    net, net_images, out = check_net(golden, "small_f64_64x64")
    check_no_host_synchronisation(net, net_images, out)
    check_estimate_depth(net)
    check_refusals(backbone, net, images)
    print("resnext torch modules ok")
