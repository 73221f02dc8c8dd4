"""Child process of tests/test_gpu_midas_grad.py::test_torch_modules (python -m tests.midas_grad_torch_child): torch is imported
first, then the library.  robust_cvd_amd.midas_train.MidasNet in .train() mode over a small stub backbone (stock-torch strided
convolutions to 16 / 21 / 40 / 72 channels, features 16), loss = (estimate_depth(net, images) * w).sum() and .backward(): p.grad of
every scratch.* parameter and of the stub backbone's weights against a stock-torch decoder with the same weights under torch's
autograd.

First the decoder cases of tests/midas_grad_cases.py through the torch layer against the f64 restatement and the CPU-minted fixture of
the reference's own MidasNet (check_fixture_net: the issue's bar, with the tie condition held by tests/test_midas_grad_reference.py).
Then estimate_depth and the stub backbone's own weights, which that fixture does not cover, against stock torch.
Bar of that second part, per gradient tensor, formed here: the stock-torch network is run twice, in f32 on the GPU and in f64 on the
CPU; delta = max |stock f32 - stock f64|, scale = max |stock f64|; |native - f64| <= 8 x max(delta, 2^-23 x scale) and |native - stock
f32| <= that bar + delta.  The seed is fixed and the head's bias keeps the output away from the last ReLU's zero (estimate_depth takes
its reciprocal); a ReLU tie that flipped between f32 and f64 would show in delta, i.e. in stock torch itself.

Also: the forward equals the forward-only class's bit for bit; (3 loss).backward() gives three times the gradients; a second backward
accumulates; a frozen native ResNeXt gets no gradient and stays in eval; a native ResNeXt that is not frozen is refused; the state-dict
keys are the forward class's; torch's synchronisation check stays silent for forward + backward, also on a side stream; one step of
robust_cvd_amd.optimizer.Adam changes every decoder parameter."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

from robust_cvd_amd import midas, midas_train, optimizer
from tests import margins
from tests import midas_cases as mc
from tests import midas_grad_cases as gc
from tests import midas_grad_reference as gr
from tests import resnext_cases as rc

DEV = torch.device("cuda", 0)
EPS32 = 2.0 ** -23
SMALL_CHANNELS = (16, 21, 40, 72)
SMALL_STUB = ((3, 16, 4), (16, 21, 2), (21, 40, 2), (40, 72, 2))      # (in, out, filter = stride) of layer1 .. layer4
FEATURES = 16


def raises(exc, call, word=None):
    try:
        call()
    except exc as e:
        assert word is None or word in str(e), (word, str(e))
    else:
        raise AssertionError(f"{exc.__name__} expected")


def small_backbone():
    backbone = torch.nn.Module()
    for i, (cin, cout, k) in enumerate(SMALL_STUB):
        setattr(backbone, f"layer{i + 1}", torch.nn.Conv2d(cin, cout, kernel_size=k, stride=k, bias=False))
    return backbone


def stock_unit(x, unit):
    r = F.relu(x)
    t = F.conv2d(r, unit.conv1.weight, unit.conv1.bias, padding=1)
    return F.conv2d(F.relu(t), unit.conv2.weight, unit.conv2.bias, padding=1) + r          # the reference's in-place ReLU


def stock_forward(net, x):
    """MidasNet.forward in stock torch ops on the modules' parameters (tools/midas_bench.py's decoder), in the parameters' dtype."""
    maps = []
    for k in (1, 2, 3, 4):
        maps.append(getattr(net.pretrained, f"layer{k}")(maps[-1] if maps else x))
    s = net.scratch
    rn = [F.conv2d(m, getattr(s, f"layer{k + 1}_rn").weight, None, padding=1) for k, m in enumerate(maps)]
    path = None
    for k in (4, 3, 2, 1):
        block = getattr(s, f"refinenet{k}")
        out = rn[k - 1]
        if path is not None:
            out = path + stock_unit(out, block.resConfUnit1)
        path = F.interpolate(stock_unit(out, block.resConfUnit2), scale_factor=2, mode="bilinear", align_corners=True)
    oc = s.output_conv
    y = F.interpolate(F.conv2d(path, oc[0].weight, oc[0].bias, padding=1), scale_factor=2, mode="bilinear", align_corners=False)
    y = F.conv2d(F.relu(F.conv2d(y, oc[2].weight, oc[2].bias, padding=1)), oc[4].weight, oc[4].bias)
    return (F.relu(y) if net.non_negative else y).squeeze(1)


def estimate(forward, images):
    """midas.estimate_depth's arithmetic around `forward`, in the images' dtype."""
    mean = torch.tensor(midas.NORM_MEAN, dtype=images.dtype, device=images.device).reshape(1, -1, 1, 1)
    stdev = torch.tensor(midas.NORM_STDEV, dtype=images.dtype, device=images.device).reshape(1, -1, 1, 1)
    return (0.0000001 + forward((images - mean) / stdev)).reciprocal()


def used(name):
    return not name.startswith("scratch.refinenet4.resConfUnit1.")       # never runs: no gradient anywhere


def grads_of(net):
    return {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}


def check_small_net(shape):
    torch.manual_seed(32103 + shape[0])
    net = midas_train.MidasNet(features=FEATURES, backbone=small_backbone(), backbone_channels=SMALL_CHANNELS)
    with torch.no_grad():
        net.scratch.output_conv[4].bias.fill_(2.0)            # the output stays away from zero: estimate_depth takes 1 / (1e-7 + y)
        net.scratch.output_conv[4].weight.abs_()
    stock64 = copy.deepcopy(net).double()                      # stock torch in f64 on the CPU: the restatement
    net = net.to(DEV).train()
    stock32 = copy.deepcopy(net)
    assert net.training and net.scratch.refinenet1.resConfUnit1.training
    rng = np.random.default_rng(shape[0] + 7)
    images = torch.from_numpy(rng.uniform(0.0, 1.0, shape).astype(np.float32))
    w = torch.from_numpy(rng.normal(0.0, 1.0, (shape[0], shape[2], shape[3])).astype(np.float32))

    # forward: the forward-only class's bits
    plain = midas.MidasNet(features=FEATURES, backbone=copy.deepcopy(net.pretrained), backbone_channels=SMALL_CHANNELS)
    assert list(plain.state_dict().keys()) == list(net.state_dict().keys())
    assert tuple(k for k in net.state_dict() if k.startswith("scratch.")) == mc.STATE_DICT_KEYS
    plain.load_state_dict(net.state_dict(), strict=True)
    plain = plain.to(DEV).eval()
    with torch.no_grad():
        want_out = midas.estimate_depth(plain, images.to(DEV))
    depth = midas.estimate_depth(net, images.to(DEV))
    assert torch.equal(depth, want_out), "the training forward differs from the forward-only class"
    assert (depth < 1e3).all(), "an output at the last ReLU's zero"
    loss = (depth * w.to(DEV)).sum()
    loss.backward()
    got = grads_of(net)
    (estimate(lambda t: stock_forward(stock32, t), images.to(DEV)) * w.to(DEV)).sum().backward()
    (estimate(lambda t: stock_forward(stock64, t), images.double()) * w.double()).sum().backward()
    ref32, ref64 = grads_of(stock32), grads_of(stock64)
    names = [n for n, _ in net.named_parameters() if used(n)]
    assert sorted(got) == sorted(names) == sorted(ref32) == sorted(ref64), "a parameter without (or with an unexpected) gradient"
    assert any(n.startswith("pretrained.") for n in names)
    for n in names:
        g, r32, r64 = got[n].cpu().double(), ref32[n].cpu().double(), ref64[n]
        assert got[n].dtype == torch.float32 and got[n].shape == ref64[n].shape and torch.isfinite(got[n]).all(), n
        delta, scale = float((r32 - r64).abs().max()), float(r64.abs().max())
        bar = 8.0 * max(delta, EPS32 * scale)
        err = float((g - r64).abs().max())
        print(f"{tuple(shape)} {n}: max |native - f64| {err:.3e}, bar {bar:.3e}, share {err / bar if bar else 0.0:.3f} (stock torch's delta {delta:.3e})")
        margins.below(f"midas train {shape[0]} {n}", err, bar)
        margins.below(f"midas train {shape[0]} {n} vs stock f32", float((g - r32).abs().max()), bar + delta)

    # a second backward accumulates: the same graph again, twice the gradient exactly
    (midas.estimate_depth(net, images.to(DEV)) * w.to(DEV)).sum().backward()
    twice = grads_of(net)
    for n in names:
        if n.startswith("scratch."):
            assert torch.equal(twice[n], got[n] + got[n]), n
        else:                                   # (the stub's weight gradient is the vendor library's: not promised to repeat bit for bit)
            assert torch.allclose(twice[n], 2 * got[n], rtol=1e-4, atol=1e-5 * float(got[n].abs().max())), n
    # (3 loss).backward(): three times the gradients, to the bar (3 gy is rounded where gy is not)
    net.zero_grad(set_to_none=True)
    (3 * (midas.estimate_depth(net, images.to(DEV)) * w.to(DEV)).sum()).backward()
    three = grads_of(net)
    for n in names:
        r64 = ref64[n]
        bar = 8.0 * max(float((ref32[n].cpu().double() - r64).abs().max()), EPS32 * float(r64.abs().max()))
        margins.below(f"midas train 3 x loss {shape[0]} {n}", float((three[n].cpu().double() - 3 * got[n].cpu().double()).abs().max()), 3 * bar)
    return net, images


def check_fixture_net(golden, name):
    """midas_train.MidasNet over the small stub of tests/midas_grad_cases.py in .train() mode, (net(images) * gy).sum().backward():
    p.grad of every scratch.* parameter and the gradients of the four feature maps within the small decoder case's bar of the f64
    restatement, and within bar + delta of the values of the reference's own MidasNet (the CPU-minted fixture)."""
    case = gc.make_small_decoder_case(name)
    maps = [torch.from_numpy(m).to(DEV).requires_grad_(True) for m in case["maps"]]        # leaves: see tests/midas_grad_cases.py: Feed
    backbone = torch.nn.Module()
    for k in range(4):
        setattr(backbone, f"layer{k + 1}", gc.Feed(maps[k]))
    net = midas_train.MidasNet(features=case["features"], non_negative=case["non_negative"], backbone=backbone, backbone_channels=gc.SMALL_CHANNELS)
    sd = net.state_dict()
    for layer in mc.STATE_DICT_LAYERS:
        w, b = case["params"][layer]
        sd[f"scratch.{layer}.weight"] = torch.from_numpy(w.copy())
        if b is not None:
            sd[f"scratch.{layer}.bias"] = torch.from_numpy(b.copy())
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).train()
    (net(torch.from_numpy(case["images"]).to(DEV)) * torch.from_numpy(case["gy"]).to(DEV)).sum().backward()
    got = {f"gm{k}": maps[k].grad.cpu().numpy() for k in range(4)}
    for i, layer in enumerate(mc.PARAMETERS):
        got[f"gw{i:02d}"] = net.scratch.get_submodule(layer).weight.grad.cpu().numpy()
        if i >= 4:
            got[f"gb{i - 4:02d}"] = net.scratch.get_submodule(layer).bias.grad.cpu().numpy()
    want = gr.decoder_grad_case(case)
    assert gc.input_digest(case) == golden[f"decoder/{name}/input_sha256"].tobytes().decode()
    assert sorted(got) == sorted(want)
    for tensor, w in want.items():
        g = got[tensor]
        key = f"decoder/{name}/{tensor}"
        delta = float(golden[key + "_delta"])
        bar = gr.bar(delta, golden[key + "_scale"])
        assert g.dtype == np.float32 and g.size == w.size
        margins.below(f"midas train fixture {name} {tensor}", np.abs(g.reshape(w.shape) - w).max(), bar)
        margins.below(f"midas train fixture {name} {tensor} vs reference", np.abs(g.reshape(-1)[case["samples"][tensor]] - golden[key]).max(),
                      bar + delta)
    print(f"{name}: 42 gradient tensors of the torch layer within the fixture's bars")


def check_frozen_native_backbone():
    torch.manual_seed(5)
    net = midas_train.MidasNet(features=FEATURES, backbone=midas.ResNeXt(*rc.SMALL), freeze_backbone=True).to(DEV)
    net.train()
    assert net.training and not net.pretrained.training and not any(m.training for m in net.pretrained.modules())
    assert not any(p.requires_grad for p in net.pretrained.parameters())
    with torch.no_grad():
        net.scratch.output_conv[4].bias.fill_(2.0)
    images = torch.rand(1, 3, 32, 32, device=DEV)
    midas.estimate_depth(net, images).sum().backward()
    assert all(p.grad is None for p in net.pretrained.parameters())
    live = 0
    for n, p in net.scratch.named_parameters():
        if used("scratch." + n):
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
            live += int((p.grad != 0).any())
    assert live >= 30, live
    raises(ValueError, lambda: midas_train.MidasNet(features=FEATURES, backbone=midas.ResNeXt(*rc.SMALL)), "no kernel yet")
    raises(ValueError, lambda: midas_train.conv2d(images, torch.zeros(4, 3, 3, 3, device=DEV), relu=True), "no differentiable path")


def check_no_host_synchronisation(net):
    """Once the handle's scratch has its size, the decoder's forward + backward are enqueued launches only: torch's synchronisation
    check stays silent, also on a side stream.  (On the feature maps: the stock-torch stub in front is the vendor library's.)"""
    torch.manual_seed(9)
    maps = [torch.randn(2, c, 16 >> k, 8 >> k, device=DEV, requires_grad=True) for k, c in enumerate(SMALL_CHANNELS)]
    w = torch.randn(2, 64, 32, device=DEV)

    def run():
        net.zero_grad(set_to_none=True)
        for m in maps:
            m.grad = None
        (net.decode(*maps) * w).sum().backward()
        return [m.grad.clone() for m in maps] + [p.grad.clone() for n, p in net.scratch.named_parameters() if p.grad is not None]
    first = run()
    torch.cuda.synchronize(DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = run()
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            third = run()
        torch.cuda.current_stream(DEV).wait_stream(side)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize(DEV)
    assert len(first) == 4 + 38
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(first, again, third)), "the gradients do not repeat bit for bit"


def check_adam_step(net, images):
    net.zero_grad(set_to_none=True)
    midas.estimate_depth(net, images.to(DEV)).sum().backward()
    params = [p for n, p in net.named_parameters() if n.startswith("scratch.") and used(n)]
    before = [p.detach().clone() for p in params]
    optimizer.Adam(params, lr=1e-3).step()
    torch.cuda.synchronize(DEV)
    assert all(torch.isfinite(p).all() and (p != b).any() for p, b in zip(params, before))


if __name__ == "__main__":
    torch.cuda.init()
    fixture = np.load(gr.GOLDEN)
    for case_name in gc.SMALL_DECODER_CASES:
        check_fixture_net(fixture, case_name)
    check_small_net((1, 3, 32, 32))
    kept = check_small_net((2, 3, 64, 32))
    check_frozen_native_backbone()
    check_no_host_synchronisation(kept[0])
    check_adam_step(*kept)
    print("midas train modules ok")
