"""Child process of tests/test_gpu_raftenc.py::test_torch_modules (python -m tests.raftenc_torch_child): torch is imported first,
then the library; robust_cvd_amd.raft_ops.BasicEncoder on GPU tensors against the array path (Solver.raft_encoder), the float64
restatement and the reference's stored values, with the bars of tests/test_gpu_raftenc.py; then robust_cvd_amd.raft_ops.RAFT against
the same network in stock torch f64 on the CPU (tests/raftenc_reference.py: stock_raft) and the reference's stored f32 flow.  With
--keys (tests/test_raftenc_reference.py; no GPU is touched): the state-dict keys only."""
import argparse
import io
import sys

import numpy as np
import torch

from robust_cvd_amd.raft_ops import RAFT, BasicEncoder, ResidualBlock
from tests import margins
from tests import raftenc_cases as ec
from tests import raftenc_reference as er


def raises(exc, call, word=None):
    try:
        call()
    except exc as e:
        assert word is None or word in str(e), (word, str(e))
    else:
        raise AssertionError(f"{exc.__name__} expected")


def args():
    return argparse.Namespace(small=False, mixed_precision=False)


def check_keys():
    golden = np.load(er.GOLDEN)
    module = RAFT(args())
    keys = list(module.state_dict().keys())
    assert keys == golden["state_dict_keys"].tolist() == list(ec.RAFT_STATE_DICT_KEYS) and len(keys) == 179, keys
    case = ec.make_raft_case("128x128")
    sd = er.raft_state_dict(case)
    result = module.load_state_dict(sd, strict=True)                        # the reference's names and shapes
    assert not result.missing_keys and not result.unexpected_keys
    assert torch.equal(module.cnet.layer2[0].norm3.running_var, sd["cnet.layer2.0.downsample.1.running_var"])
    assert module.cnet.layer2[0].downsample[1] is module.cnet.layer2[0].norm3
    # as the reference loads a checkpoint: saved from a DataParallel wrapper, loaded into one, used through .module
    buf = io.BytesIO()
    torch.save({"module." + k: v for k, v in sd.items()}, buf)
    buf.seek(0)
    wrapped = torch.nn.DataParallel(RAFT(args()))
    result = wrapped.load_state_dict(torch.load(buf), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert torch.equal(wrapped.module.fnet.conv2.bias, sd["fnet.conv2.bias"])
    assert list(BasicEncoder(256, "instance").state_dict().keys()) == ec.encoder_keys("", "instance")
    assert list(BasicEncoder(256, "batch").state_dict().keys()) == ec.encoder_keys("", "batch")
    raises(ValueError, lambda: BasicEncoder(norm_fn="group"), "group")
    raises(ValueError, lambda: ResidualBlock(64, 64, "group"), "group")
    raises(ValueError, lambda: RAFT(argparse.Namespace(small=True)), "small")
    print("raft state dict keys ok")


if __name__ == "__main__" and "--keys" in sys.argv:
    check_keys()
    sys.exit(0)

from robust_cvd_amd import torch_common as tc  # noqa: E402

DEV = torch.device("cuda", 0)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def encoder_of(case):
    module = BasicEncoder(output_dim=ec.OUTPUT_DIM, norm_fn=case["norm_mode"], dropout=0.0)
    result = module.load_state_dict(er.encoder_state_dict(case), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    return module.to(DEV).eval()


def check_encoder(solver, golden, name):
    case = ec.make_encoder_case(name)
    module = encoder_of(case)
    images = gpu(case["images"])
    with torch.no_grad():
        out = module(images)
    array = solver.raft_encoder(case["images"], case["weights"], case["biases"], norm=case["norm_mode"],
                                norms=case["norms"] if case["norm_mode"] == "batch" else None, eps=ec.EPS)
    want = er.encoder_case(case)
    got = out.cpu().numpy()
    assert tuple(out.shape) == want.shape and out.dtype == torch.float32 and out.is_contiguous()
    assert np.array_equal(got, array), name                                 # the same kernels through the array path: bit for bit
    delta = float(golden[f"encoder/{name}/out_delta"])
    bar = er.bar(delta, golden[f"encoder/{name}/out_scale"])
    margins.below(f"raft encoder torch {name}", np.abs(got - want).max(), bar)
    margins.below(f"raft encoder torch {name} vs reference",
                  np.abs(ec.sample_view(got, case["samples"]) - golden[f"encoder/{name}/out"]).max(), bar + delta)
    with torch.no_grad():
        # the list form: two tensors in, two out, each what the image gives on its own (B = 1 here, so also against one by one)
        a, b = images, torch.flip(images, dims=(3,)).contiguous()
        fa, fb = module([a, b])
        assert torch.equal(fa, out) and torch.equal(fb, module(b)) and fa.shape == out.shape
    return module, images, out


def check_blocks(solver):
    """ResidualBlock on its own against the encoder's stages through the array path, bit for bit."""
    for name in ("instance_16x24b3", "batch_16x24b3", "none_16x24b3"):
        case = ec.make_encoder_case(name)
        module = encoder_of(case)
        rng = np.random.default_rng(5)
        x = np.maximum(rng.normal(0, 1, (2, 64, 8, 12)), 0).astype(np.float32)
        with torch.no_grad():
            got = module.layer2(gpu(x)).cpu().numpy()
        mode, w, b, n = case["norm_mode"], case["weights"], case["biases"], case["norms"]

        def layer(i, t, relu, residual=None):
            stride = ec.LAYERS[i][4]
            if mode == "instance":
                y = solver.raft_encoder_conv(t, w[i], b[i], stride=stride)
                return solver.raft_instance_norm(y, eps=ec.EPS, relu=relu, residual=residual, inplace=True)
            return solver.raft_encoder_conv(t, w[i], b[i], stride=stride, norm=n[i] if mode == "batch" else None, eps=ec.EPS, relu=relu,
                                            residual=residual)
        y = layer(6, layer(5, x, True), True, layer(7, x, False))
        y = layer(9, layer(8, y, True), True, y)
        assert np.array_equal(got, y), name


def raft_of(case):
    module = RAFT(args())
    result = module.load_state_dict(er.raft_state_dict(case), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    return module.to(DEV).eval()


def check_raft(golden, name):
    case = ec.make_raft_case(name)
    assert ec.input_digest(case) == golden[f"raft/{name}/input_sha256"].tobytes().decode()
    module = raft_of(case)
    i1, i2 = torch.from_numpy(case["image1"]), torch.from_numpy(case["image2"])
    low64, up64 = er.stock_raft(er.raft_state_dict(case), i1, i2, case["iters"], torch.float64)
    with torch.no_grad():
        low, up = module(i1.to(DEV), i2.to(DEV), iters=case["iters"], test_mode=True)
    for o, got, want, samples in (("flow_low", low, low64, case["samples_low"]), ("flow_up", up, up64, case["samples_up"])):
        assert got.shape == want.shape and got.dtype == torch.float32
        delta = float(golden[f"raft/{name}/{o}_delta"])
        scale = float(golden[f"raft/{name}/{o}_scale"])
        assert abs(scale - float(want.abs().max())) <= 1e-6 * scale
        bar = er.bar(delta, scale)
        err = float((got.cpu().double() - want).abs().max())
        print(f"raft {name} {o}: max |kernels - f64| {err:.3e}, bar {bar:.3e}, share {err / bar:.3f} (reference's own delta {delta:.3e})")
        margins.below(f"raft {name} {o}", err, bar)
        margins.below(f"raft {name} {o} vs reference",
                      np.abs(ec.sample_view(got.cpu().numpy(), samples) - golden[f"raft/{name}/{o}"]).max(), bar + delta)
    return module, i1.to(DEV), i2.to(DEV), (low, up)


def check_forms(module, i1, i2, outs, iters):
    low, up = outs
    with torch.no_grad():
        # the list form: every iteration's upsampled flow, the last the test mode's; with every mask computed the bits are the same
        flows = module(i1, i2, iters=iters)
        assert isinstance(flows, list) and len(flows) == iters and torch.equal(flows[-1], up)
        again = module(i1, i2, iters=iters, upsample=False, test_mode=True)
        assert torch.equal(again[0], low) and torch.equal(again[1], up)
        # flow_init: a zero one changes nothing; the 1/8 flow as the start of one more iteration against the stock f64 network, the
        # bar from the stock f32 network's own error
        zero = module(i1, i2, iters=iters, flow_init=torch.zeros_like(low), test_mode=True)
        assert torch.equal(zero[0], low) and torch.equal(zero[1], up)
        warm = module(i1, i2, iters=1, flow_init=low, test_mode=True)
        assert torch.isfinite(warm[1]).all() and warm[0].shape == low.shape
        sd = {k: v.cpu() for k, v in module.state_dict().items()}
        want = er.stock_raft(sd, i1.cpu(), i2.cpu(), 1, torch.float64, flow_init=low.cpu())
        own = er.stock_raft(sd, i1.cpu(), i2.cpu(), 1, torch.float32, flow_init=low.cpu())
        for got, w64, w32 in zip(warm, want, own):
            delta, scale = float((w32.double() - w64).abs().max()), float(w64.abs().max())
            margins.below("raft flow_init", float((got.cpu().double() - w64).abs().max()), er.bar(delta, scale))


def check_no_host_synchronisation(module, i1, i2, outs, iters):
    """Once the handle's scratch has its size a call is enqueued launches only: torch's synchronisation check stays silent, also on
    a side stream."""
    torch.cuda.synchronize(DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            again = module(i1, i2, iters=iters, test_mode=True)
            side = torch.cuda.Stream(device=DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                third = module(i1, i2, iters=iters, test_mode=True)
            torch.cuda.current_stream(DEV).wait_stream(side)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize(DEV)
    for a, b, c in zip(again, third, outs):
        assert torch.equal(a, c) and torch.equal(b, c)


def check_refusals(module, i1, i2):
    enc = module.fnet
    x = (2 * (i1 / 255.0) - 1.0).contiguous()
    with torch.no_grad():
        raises(ValueError, lambda: module(i1.cpu(), i2), "GPU")
        raises(TypeError, lambda: module(i1.double(), i2), "float32")
        raises(TypeError, lambda: module(i1, i2.half()), "float32")
        raises(ValueError, lambda: module(i1[:, :, :-4], i2[:, :, :-4]), "multiples of 8")
        raises(ValueError, lambda: module(i1[:, :, :, :-3], i2[:, :, :, :-3]), "multiples of 8")
        raises(ValueError, lambda: module(i1[:, :, :120], i2[:, :, :120]), "16 x 16")
        raises(ValueError, lambda: module(i1, i2[:, :, :64]), "alike")
        raises(ValueError, lambda: module(i1, i2, flow_init=torch.zeros(1, 2, 3, 3, device=DEV)), "flow_init must be")
        raises(ValueError, lambda: RAFT(args()).eval()(i1, i2), "different devices")                  # parameters on the CPU
        raises(ValueError, lambda: enc(x.cpu()), "GPU")
        raises(TypeError, lambda: enc(x.double()), "float32")
        raises(ValueError, lambda: enc([x, x, x]), "two tensors")
        raises(ValueError, lambda: enc(x[:, :2]), "(B, 3, H, W)")
        raises(ValueError, lambda: enc(x[:, :, :8, :8]), "more than 1 spatial element")
        raises(ValueError, lambda: BasicEncoder(256, "batch").to(DEV)(x), "training mode")          # a fresh module is in training mode
        raises(ValueError, lambda: BasicEncoder(256, "instance", dropout=0.5).to(DEV)(x), "dropout")
        assert BasicEncoder(256, "instance", dropout=0.5).to(DEV).eval()(x).shape == (x.shape[0], 256, x.shape[2] // 8, x.shape[3] // 8)
        # training mode with the batch norms frozen is legal, as the reference trains
        module.train()
        raises(ValueError, lambda: module(i1, i2, iters=1), "training mode")
        module.freeze_bn()
        assert len(module(i1, i2, iters=1)) == 1
        module.eval()
    # grad mode on: the parameters require grad
    raises(ValueError, lambda: module(i1, i2, iters=1), "forward only")
    raises(ValueError, lambda: enc(x), "forward only")
    for p in module.parameters():
        p.requires_grad_(False)
    raises(ValueError, lambda: module(i1.clone().requires_grad_(True), i2, iters=1), "forward only")
    torch.cuda.synchronize(DEV)
    assert module(i1, i2, iters=1)[0].shape == i1.shape[:1] + (2,) + i1.shape[2:]
    if torch.cuda.device_count() > 1:
        raises(ValueError, lambda: module(i1, i2.to("cuda:1"), iters=1), "different devices")
    torch.cuda.synchronize(DEV)


if __name__ == "__main__":
    torch.cuda.init()
    golden = np.load(er.GOLDEN)
    solver = tc.solver(DEV)
    for name in ("instance_40x56", "batch_40x56", "instance_9x9", "none_16x24b3"):
        check_encoder(solver, golden, name)
    # fnet([a, b]) against fnet(a), fnet(b) at B = 3
    case = ec.make_encoder_case("instance_16x24b3")
    module = encoder_of(case)
    with torch.no_grad():
        a = gpu(case["images"])
        b = torch.flip(a, dims=(2,)).contiguous()
        fa, fb = module([a, b])
        assert torch.equal(fa, module(a)) and torch.equal(fb, module(b))
        for i in range(3):
            assert torch.equal(module(a[i:i + 1])[0], fa[i])
    check_blocks(solver)
    kept = None
    for name in ec.RAFT_CASES:
        kept = check_raft(golden, name) + (ec.RAFT_CASES[name][1],)
        if name == "128x128":
            check_forms(*kept)
    check_no_host_synchronisation(*kept)
    check_refusals(*kept[:3])
    print("raft encoder torch modules ok")
