"""Child process of tests/test_gpu_resnext_grad.py::test_torch_layer_in_a_fresh_process: torch is imported first, then the library.
robust_cvd_amd.midas_train.ResNeXt on the GPU against the same backbone in STOCK TORCH ops (tests/resnext_reference.py: stock_resnet)
under torch's autograd on the CPU.

Whole backbone, SMALL = ((2, 1, 2, 1), 4, 8) at 2 x 3 x 64 x 64 in training mode, loss = sum_k <w_k, map_k> with seeded weights: every
parameter gradient, the four feature maps and the updated running statistics.  Bar per tensor, formed here: the stock network runs
twice on the CPU, in f32 and in f64; delta = max |stock f32 - stock f64|, scale = max |stock f64|; |native - f64| <= 8 x max(delta,
2^-23 x scale).  Condition against a vacuous bar: delta <= 1e-4 x scale for every tensor (a ReLU or pool tie that flipped between
f32 and f64 would show in delta, i.e. in stock torch itself); the draw of tests/resnext_grad_cases.py meets it, or this fails.

Also: the eval-mode (frozen statistics) backward against stock torch in eval mode; num_batches_tracked; a repeat is bit for bit;
under no_grad in eval mode the forward is the forward-only class's bit for bit; midas_train.MidasNet over the trainable backbone
loads the backbone's and the decoder's keys with strict=True; p.grad of every pretrained.* and scratch.* parameter against the
reference's MidasNet.forward in stock torch ops over the stock backbone (CPU, f32 and f64, the same bar and condition); it stays
finite through three steps of robust_cvd_amd.optimizer.Adam; the real depth (3, 4, 23, 3) at 1 x 3 x 64 x 64 is finite and repeats bit for bit."""
import copy

import numpy as np
import torch

from robust_cvd_amd import api, midas, midas_train, optimizer
from tests import margins
from tests import midas_cases as mc
from tests.midas_grad_torch_child import stock_forward
from tests import resnext_cases as rc
from tests import resnext_grad_cases as gc
from tests import resnext_reference as rr

DEV = torch.device("cuda", 0)
EPS32 = 2.0 ** -23


def stock_run(case, dtype, train):
    """The stock backbone on the CPU in `dtype`: (maps, {tv parameter name: grad}, {buffer name: value after the forward})."""
    resnet = rr.stock_resnet(case["blocks"], case["groups"], case["width_per_group"])
    rr.load_parameters(resnet, case["params"], case["blocks"], case["groups"], case["width_per_group"])
    net = rr.midas_backbone(resnet).to(dtype).train(train)
    x = torch.from_numpy(case["images"]).to(dtype)
    maps = []
    for k in range(4):
        x = getattr(net, f"layer{k + 1}")(x)
        maps.append(x)
    loss = sum((m * torch.from_numpy(w).to(dtype)).sum() for m, w in zip(maps, case["loss_weights"]))
    loss.backward()
    grads = {n: p.grad.double().numpy() for n, p in resnet.named_parameters()}
    stats = {n: b.double().numpy() for n, b in resnet.named_buffers() if not n.endswith("num_batches_tracked")}
    return [m.detach().double().numpy() for m in maps], grads, stats


def native_backbone(case):
    net = midas_train.ResNeXt(case["blocks"], case["groups"], case["width_per_group"])
    sd = {k[len("pretrained."):]: v for k, v in rr.pretrained_state_dict(case).items()}
    result = net.load_state_dict(sd, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    return net.to(DEV)


def native_run(case, train):
    net = native_backbone(case).train(train)
    maps = net(torch.from_numpy(case["images"]).to(DEV))
    loss = sum((m * torch.from_numpy(w).to(DEV)).sum() for m, w in zip(maps, case["loss_weights"]))
    loss.backward()
    torch.cuda.synchronize()
    return net, [m.detach().cpu().numpy() for m in maps]


def compare(label, got, f32, f64):
    delta, scale = float(np.abs(f32 - f64).max()), float(np.abs(f64).max())
    assert delta <= 1e-4 * scale, (label, "the draw misses the condition against a vacuous bar", delta, scale)
    bar = 8.0 * max(delta, EPS32 * scale)
    err = float(np.abs(got.astype(np.float64) - f64).max())
    print(f"{label}: max |native - f64| {err:.3e}, bar {bar:.3e}, share {err / bar:.3f} (stock f32's own delta {delta:.3e})")
    margins.below(f"resnext grad torch {label}", err, bar)


def names(case):
    """(torchvision name, name under midas's layer1 Sequential) of every convolution and norm of the case."""
    out = []
    for conv, norm, key, norm_key, *_ in rc.conv_table(case["blocks"], case["groups"], case["width_per_group"]):
        out += [(conv + ".weight", key + ".weight"), (norm + ".weight", norm_key + ".weight"), (norm + ".bias", norm_key + ".bias")]
    return out


def check_backbone(case, train):
    mode = "train" if train else "eval"
    maps32, grads32, stats32 = stock_run(case, torch.float32, train)
    maps64, grads64, stats64 = stock_run(case, torch.float64, train)
    net, maps = native_run(case, train)
    for k in range(4):
        compare(f"{mode} map {k + 1}", maps[k], maps32[k], maps64[k])
    params = dict(net.named_parameters())
    for tv, md in names(case):
        assert params[md].grad is not None, md
        compare(f"{mode} grad {md}", params[md].grad.cpu().numpy(), grads32[tv], grads64[tv])
    buffers = dict(net.named_buffers())
    for conv, norm, key, norm_key, *_ in rc.conv_table(case["blocks"], case["groups"], case["width_per_group"]):
        for v in ("running_mean", "running_var"):
            got = buffers[f"{norm_key}.{v}"].cpu().numpy()
            if train:
                compare(f"{mode} {norm_key}.{v}", got, stats32[f"{norm}.{v}"], stats64[f"{norm}.{v}"])
            else:
                assert np.array_equal(got.astype(np.float64), stats64[f"{norm}.{v}"]), "eval mode changed the running statistics"
        assert int(buffers[f"{norm_key}.num_batches_tracked"]) == (1 if train else 0)
    return net, maps


def grads_of(net):
    return [p.grad.clone() for p in net.parameters()]


def main():
    torch.manual_seed(0)
    case = gc.make_backbone_case()
    net, maps = check_backbone(case, True)
    # a repeat from the same state is bit for bit
    again, maps2 = native_run(case, True)
    assert all(np.array_equal(a, b) for a, b in zip(maps, maps2))
    assert all(torch.equal(a, b) for a, b in zip(grads_of(net), grads_of(again))), "a repeat differs"
    assert all(torch.equal(a, b) for a, b in zip(net.buffers(), again.buffers()))
    # frozen statistics: .eval() with parameters that require grad
    check_backbone(case, False)
    # eval mode under no_grad keeps the forward-only class's one-call path and its bits
    plain = midas.ResNeXt(case["blocks"], case["groups"], case["width_per_group"])
    plain.load_state_dict(native_backbone(case).state_dict(), strict=True)
    plain = plain.to(DEV).eval()
    trained = native_backbone(case).eval()
    x = torch.from_numpy(case["images"]).to(DEV)
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(plain(x), trained(x)))
    # refusals are _check's
    for call, exc in ((lambda: trained.train()(x.cpu()), ValueError), (lambda: trained.train()(x.double()), TypeError)):
        try:
            call()
        except exc:
            pass
        else:
            raise AssertionError(f"{exc.__name__} expected")

    # the whole network, every parameter trainable
    features = 64
    rng = np.random.default_rng(33011)
    full = midas_train.MidasNet(backbone=midas_train.ResNeXt(*rc.SMALL), features=features, non_negative=False)
    sd = rr.pretrained_state_dict(case)
    sd.update(rr.scratch_state_dict({"decoder": mc.decoder_parameters(rng, features)}))
    result = full.load_state_dict(sd, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert [k for k in full.state_dict() if k.startswith("pretrained.")] == api.resnext_state_dict_keys(*rc.SMALL)
    weight = torch.from_numpy(rng.normal(0.0, 1.0, (2, 64, 64)).astype(np.float32))
    # the same network in stock torch ops on the CPU, in f32 and in f64: the reference's MidasNet.forward over the stock backbone
    # (tests/midas_grad_torch_child.py: stock_forward), batch-statistics norms, every parameter trained
    stock = {}
    for dtype in (torch.float32, torch.float64):
        resnet = rr.stock_resnet(*rc.SMALL)
        net = midas_train.MidasNet(backbone=rr.midas_backbone(resnet), features=features, non_negative=False)
        result = net.load_state_dict(sd, strict=True)
        assert not result.missing_keys and not result.unexpected_keys
        net = net.to(dtype).train()
        (stock_forward(net, torch.from_numpy(case["images"]).to(dtype)) * weight.to(dtype)).sum().backward()
        stock[dtype] = {n: p.grad.double().numpy() for n, p in net.named_parameters() if p.grad is not None}
    weight = weight.to(DEV)
    full = full.to(DEV).train()
    unused = "scratch.refinenet4.resConfUnit1."          # (the reference's refinenet4 takes one input: that unit never runs)
    opt = optimizer.Adam([p for n, p in full.named_parameters() if not n.startswith(unused)], lr=1e-4)
    for step in range(3):
        opt.zero_grad()
        out = full(x)
        (out * weight).sum().backward()
        if step == 0:
            for n, p in full.named_parameters():
                if n.startswith(unused):
                    assert p.grad is None, n
                    continue
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
                compare(f"MidasNet grad {n}", p.grad.cpu().numpy(), stock[torch.float32][n], stock[torch.float64][n])
            assert sum(n.startswith("pretrained.") for n, _ in full.named_parameters()) == len(names(case))
        opt.step()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in full.parameters()) and bool(torch.isfinite(out).all())
    assert int(full.pretrained.layer1[1].num_batches_tracked) == 3

    # the real depth: finite and repeating (ties make a comparison against stock torch meaningless at random weights)
    real_case = {"blocks": rc.REAL[0], "groups": rc.REAL[1], "width_per_group": rc.REAL[2]}
    params = rc.backbone_parameters(np.random.default_rng(33012), *rc.REAL)
    real = midas_train.resnext101_32x8d()
    sd = {k[len("pretrained."):]: v for k, v in rr.pretrained_state_dict(dict(real_case, params=params)).items()}
    real.load_state_dict(sd, strict=True)
    runs = []
    for _ in range(2):
        net = copy.deepcopy(real).to(DEV).train()
        outs = net(x[:1])
        sum(o.sum() for o in outs).backward()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
        runs.append(grads_of(net))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "the real depth does not repeat"
    print("all checks passed")


if __name__ == "__main__":
    main()
