"""Mints midas_grad_golden.npz on the CPU under torch's autograd (f32), never from the project's kernels:

    python -m tests.golden.reference_py.make_midas_grad_golden

Per seeded case of tests/midas_grad_cases.py and per gradient tensor: torch's f32 gradient at the case's <= 16 sampled elements,
delta = max |torch f32 - float64 restatement| over the WHOLE tensor, scale = max |restatement|, and the digest of the inputs (the
inputs are not stored).  A convolution is the nn.Conv2d the reference's blocks.py and midas_net.py build (stride 1, padding k // 2):
its input gradient is the leaf's .grad after backward(gy), then the addend and the mask in the kernel's stated epilogue order; its
weight and bias gradients are the module's parameters' .grad with the input rectified first under relu_in.  The upsampling is
nn.functional.interpolate(align_corners=True) as FeatureFusionBlock calls it, resp. the reference's own Interpolate class
(tests/midas_reference.py: load_reference).  The head is the reference network's own scratch.output_conv[2:] over the stub backbone
(reference_net there); for its two rectified tensors the fixture also records torch's f32 error and whether every f32 sign agrees
with the restatement's (the tie condition of the cases whose masks are computed)."""
import numpy as np
import torch

from tests import midas_grad_cases as gc
from tests import midas_cases as mc
from tests import midas_grad_reference as gr
from tests import midas_reference as mr


def t(a):
    return torch.from_numpy(np.array(a))


def store(out, key, case, refs, wants):
    for name, want in wants.items():
        ref = refs[name]
        assert ref.shape == want.shape and ref.dtype == np.float32, (key, name)
        out[f"{key}/{name}"] = ref.reshape(-1)[case["samples"][name]]
        out[f"{key}/{name}_delta"] = np.float64(np.abs(ref.astype(np.float64) - want).max())
        out[f"{key}/{name}_scale"] = np.float64(np.abs(want).max())
    out[f"{key}/input_sha256"] = np.frombuffer(gc.input_digest(case).encode(), np.uint8)


def reference_conv_grads(case):
    w = case["weight"]
    conv = torch.nn.Conv2d(w.shape[1], w.shape[0], case["k"], padding=case["k"] // 2, bias=True)
    conv.load_state_dict({"weight": t(w), "bias": torch.zeros(w.shape[0])})
    # the input gradient: of the convolution itself (the input ReLU's mask is the operator's `mask`)
    leaf = t(case["x"]).requires_grad_(True)
    conv(leaf).backward(t(case["gy"]))
    gx = leaf.grad.detach()
    if case["add"] is not None:
        gx = gx + t(case["add"])
    if case["mask"] is not None:
        gx = torch.where(t(case["mask"]) > 0, gx, torch.zeros_like(gx))
    # the weight and bias gradients: with the input rectified first under relu_in
    conv.zero_grad()
    x = t(case["x"])
    conv(torch.relu(x) if case["relu_in"] else x).backward(t(case["gy"]))
    return {"gx": gx.numpy(), "gw": conv.weight.grad.numpy(), "gb": conv.bias.grad.numpy()}


def reference_small_decoder(reference, case):
    """({gw.., gb.., gm..} of the reference's MidasNet under autograd, {name: the rectified tensors of gr.rectified in f32})."""
    blocks, midas_net = reference
    # the four feature maps enter as leaves (a stage that returns its stored map, whatever it is given): their .grad is then the
    # decoder's hand-over alone, without what flows on through the next backbone stage
    maps = [t(m).requires_grad_(True) for m in case["maps"]]
    backbone = torch.nn.Module()
    for k in range(4):
        setattr(backbone, f"layer{k + 1}", gc.Feed(maps[k]))
    midas_net._make_encoder = lambda f, use_pretrained: (backbone, blocks._make_scratch(list(gc.SMALL_CHANNELS), f))
    net = midas_net.MidasNet(path=None, features=case["features"], non_negative=case["non_negative"]).train()
    sd = net.state_dict()
    for layer in mc.STATE_DICT_LAYERS:
        w, b = case["params"][layer]
        sd[f"scratch.{layer}.weight"] = t(w)
        if b is not None:
            sd[f"scratch.{layer}.bias"] = t(b)
    net.load_state_dict(sd, strict=True)
    captured = {}
    keep = lambda key: (lambda _m, _i, o: captured.__setitem__(key, o.detach().clone().numpy()))
    keep_in = lambda key: (lambda _m, i: captured.__setitem__(key, i[0].detach().clone().numpy()))
    for k in range(4):
        block = getattr(net.scratch, f"refinenet{k + 1}")
        block.resConfUnit2.register_forward_pre_hook(keep_in(f"o{k}"))
        block.resConfUnit2.conv1.register_forward_hook(keep(f"t2_{k}"))
        if k < 3:
            block.resConfUnit1.register_forward_pre_hook(keep_in(f"rn{k}"))
            block.resConfUnit1.conv1.register_forward_hook(keep(f"t1_{k}"))
    net.scratch.output_conv[2].register_forward_hook(keep("t"))
    net.scratch.output_conv[4].register_forward_hook(lambda _m, _i, o: captured.__setitem__("s", o.detach().clone().numpy()[:, 0]))
    y = net(t(case["images"]))
    y.backward(t(case["gy"]))
    refs = {}
    for i, layer in enumerate(mc.PARAMETERS):
        refs[f"gw{i:02d}"] = net.scratch.get_submodule(layer).weight.grad.numpy()
        if i >= 4:
            refs[f"gb{i - 4:02d}"] = net.scratch.get_submodule(layer).bias.grad.numpy()
    refs.update({f"gm{k}": maps[k].grad.numpy() for k in range(4)})
    assert all(p.grad is None for n, p in net.scratch.named_parameters() if n.startswith("refinenet4.resConfUnit1."))
    return refs, captured


def main():
    reference = mr.load_reference()
    assert reference is not None, "the reference checkout is not available"
    blocks, _midas_net = reference
    out = {}
    for name in gc.CONV_GRAD_CASES:
        case = gc.make_conv_grad_case(name)
        store(out, "conv/" + name, case, reference_conv_grads(case), gr.conv_grad_case(case))
    for name in gc.UPSAMPLE_GRAD_CASES:
        case = gc.make_upsample_grad_case(name)
        B, Cn, Ho, Wo = case["gy"].shape
        leaf = torch.zeros(B, Cn, Ho // 2, Wo // 2, requires_grad=True)
        if case["align_corners"]:
            y = torch.nn.functional.interpolate(leaf, scale_factor=2, mode="bilinear", align_corners=True)
        else:
            y = blocks.Interpolate(scale_factor=2, mode="bilinear")(leaf)
        y.backward(t(case["gy"]))
        store(out, "upsample/" + name, case, {"gx": leaf.grad.numpy()}, gr.upsample_grad_case(case))
    # the head: the reference network's own output_conv[2:] (midas_net.py:38-41), as the forward's fixture takes it
    nets = {}
    for name in ("f64_64x64", "f256_96x64b2"):
        dcase = mc.make_decoder_case(name)
        nets[dcase["non_negative"]] = mr.reference_net(reference, dcase)
    for name in gc.HEAD_GRAD_CASES:
        case = gc.make_head_grad_case(name)
        tail = nets[case["non_negative"]].scratch.output_conv[2:]
        tail.load_state_dict({"2.weight": t(case["weight2"]), "2.bias": t(case["bias2"]), "4.weight": t(case["weight4"]),
                              "4.bias": t(case["bias4"])}, strict=True)
        tail.zero_grad()
        leaf = t(case["x"]).requires_grad_(True)
        tail(leaf)[:, 0].backward(t(case["gy"]))
        refs = {"gx": leaf.grad.numpy(), "gw2": tail[0].weight.grad.numpy(), "gb2": tail[0].bias.grad.numpy(),
                "gw4": tail[2].weight.grad.numpy(), "gb4": tail[2].bias.grad.numpy()}
        store(out, "head/" + name, case, refs, gr.head_grad_case(case))
        # the tie condition: the forward's two rectified tensors in torch's f32 against the f64 restatement
        with torch.no_grad():
            t32 = tail[0](t(case["x"])).numpy()
            s32 = tail[2](torch.relu(t(t32)))[:, 0].numpy()
        for tensor, got32, want in zip(("t", "s"), (t32, s32), gr.head_forward(case)):
            out[f"head/{name}/{tensor}_delta"] = np.float64(np.abs(got32.astype(np.float64) - want).max())
            out[f"head/{name}/{tensor}_scale"] = np.float64(np.abs(want).max())
            out[f"head/{name}/{tensor}_signs_agree"] = np.bool_(((got32 > 0) == (want > 0)).all())
            print(name, tensor, "min |value|", float(np.abs(want).min()), "signs agree", bool(out[f"head/{name}/{tensor}_signs_agree"]),
                  "share <= 0", float((want <= 0).mean()))
    # small whole decoders: the reference's own MidasNet (blocks.py's _make_scratch, ResidualConvUnit, FeatureFusionBlock, Interpolate)
    # over the small stub backbone, under autograd; its rectified tensors are captured by hooks (cloned: its ReLUs are in place)
    for name in gc.SMALL_DECODER_CASES:
        case = gc.make_small_decoder_case(name)
        refs, captured = reference_small_decoder(reference, case)
        store(out, "decoder/" + name, case, refs, gr.decoder_grad_case(case))
        for tensor, want in gr.rectified(gr.decoder_forward(case)).items():
            got32 = captured[tensor]
            assert got32.shape == want.shape, (name, tensor)
            out[f"decoder/{name}/{tensor}_delta"] = np.float64(np.abs(got32.astype(np.float64) - want).max())
            out[f"decoder/{name}/{tensor}_scale"] = np.float64(np.abs(want).max())
            out[f"decoder/{name}/{tensor}_signs_agree"] = np.bool_(((got32 > 0) == (want > 0)).all())
            print(name, tensor, "min |value|", float(np.abs(want).min()), "bar", gr.bar(out[f"decoder/{name}/{tensor}_delta"], np.abs(want).max()),
                  "signs agree", bool(out[f"decoder/{name}/{tensor}_signs_agree"]))
    for key in sorted(k for k in out if k.endswith("_delta")):
        print(key, float(out[key]), float(out[key.replace("_delta", "_scale")]))
    np.savez_compressed(gr.GOLDEN, **out)


if __name__ == "__main__":
    main()
