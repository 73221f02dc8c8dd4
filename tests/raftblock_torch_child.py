"""Child process of tests/test_gpu_raftblock.py::test_torch_module (python -m tests.raftblock_torch_child): torch is imported
first, then the library; robust_cvd_amd.raft_ops.BasicUpdateBlock on GPU tensors against the array path
(Solver.raft_update_block), the float64 restatement and the reference's stored values, with the bars of
tests/test_gpu_raftblock.py; then two refinement iterations CorrBlock -> BasicUpdateBlock -> upsample_flow against the same loop in
stock torch f64 on the CPU.  With --keys (tests/test_raftblock_reference.py; no GPU is touched): the state-dict keys only."""
import io
import sys

import numpy as np
import torch
import torch.nn.functional as F

from robust_cvd_amd.raft_ops import BasicMotionEncoder, BasicUpdateBlock, CorrBlock, FlowHead, upsample_flow
from tests import margins
from tests import raftblock_cases as bc
from tests import raftblock_reference as br


def raises(exc, call, word=None):
    try:
        call()
    except exc as e:
        assert word is None or word in str(e), (word, str(e))
    else:
        raise AssertionError(f"{exc.__name__} expected")


class StockBlock(torch.nn.Module):
    """BasicUpdateBlock written with stock torch ops, in the reference's layout (its parameter names and shapes; formulas of
    raft/core/update.py restated, `gru` any module with the reference's SepConvGRU parameters)."""

    class Encoder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.convc1 = torch.nn.Conv2d(bc.COR_PLANES, 256, 1)
            self.convc2 = torch.nn.Conv2d(256, 192, 3, padding=1)
            self.convf1 = torch.nn.Conv2d(2, 128, 7, padding=3)
            self.convf2 = torch.nn.Conv2d(128, 64, 3, padding=1)
            self.conv = torch.nn.Conv2d(256, 126, 3, padding=1)

        def forward(self, flow, corr):
            cor = F.relu(self.convc2(F.relu(self.convc1(corr))))
            flo = F.relu(self.convf2(F.relu(self.convf1(flow))))
            return torch.cat([F.relu(self.conv(torch.cat([cor, flo], 1))), flow], 1)

    class Gru(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for half, k in ((1, (1, 5)), (2, (5, 1))):
                for g in "zrq":
                    setattr(self, f"conv{g}{half}", torch.nn.Conv2d(384, 128, k, padding=(k[0] // 2, k[1] // 2)))

        def forward(self, h, x):
            for half in (1, 2):
                hx = torch.cat([h, x], 1)
                z = torch.sigmoid(getattr(self, f"convz{half}")(hx))
                r = torch.sigmoid(getattr(self, f"convr{half}")(hx))
                q = torch.tanh(getattr(self, f"convq{half}")(torch.cat([r * h, x], 1)))
                h = (1 - z) * h + z * q
            return h

    class Head(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = torch.nn.Conv2d(128, 256, 3, padding=1)
            self.conv2 = torch.nn.Conv2d(256, 2, 3, padding=1)

        def forward(self, x):
            return self.conv2(F.relu(self.conv1(x)))

    def __init__(self):
        super().__init__()
        self.encoder, self.gru, self.flow_head = self.Encoder(), self.Gru(), self.Head()
        self.mask = torch.nn.Sequential(torch.nn.Conv2d(128, 256, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(256, 576, 1))

    def forward(self, net, inp, corr, flow):
        net = self.gru(net, torch.cat([inp, self.encoder(flow, corr)], 1))
        return net, 0.25 * self.mask(net), self.flow_head(net)


def check_keys():
    golden = np.load(br.GOLDEN)
    module = BasicUpdateBlock(br.Args(), hidden_dim=128, input_dim=128)
    keys = list(module.state_dict().keys())
    assert keys == golden["state_dict_keys"].tolist() == list(bc.STATE_DICT_KEYS), keys
    assert keys == list(StockBlock().state_dict().keys())
    case = bc.make_block_case("1x1")
    result = module.load_state_dict(br.state_dict(case), strict=True)       # the reference's names and shapes
    assert not result.missing_keys and not result.unexpected_keys
    assert torch.equal(module.mask[2].bias, torch.from_numpy(case["biases"][14]))
    assert tuple(BasicUpdateBlock().encoder.convc1.weight.shape) == (256, 324, 1, 1)
    raises(ValueError, lambda: BasicUpdateBlock(hidden_dim=96), "hidden_dim")
    raises(ValueError, lambda: BasicUpdateBlock(input_dim=256), "input_dim")
    print("raft block state dict keys ok")


if __name__ == "__main__" and "--keys" in sys.argv:
    check_keys()
    sys.exit(0)

from robust_cvd_amd import torch_common as tc  # noqa: E402

DEV = torch.device("cuda", 0)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def module_of(case):
    """The drop-in with the case's parameters, loaded through a state dict SAVED from a stock-torch module of the same layout."""
    stock = StockBlock()
    stock.load_state_dict(br.state_dict(case))
    buf = io.BytesIO()
    torch.save(stock.state_dict(), buf)
    buf.seek(0)
    block = BasicUpdateBlock(br.Args(), hidden_dim=128, input_dim=128)
    result = block.load_state_dict(torch.load(buf), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    return block.to(DEV)


def check_case(solver, golden, name):
    case = bc.make_block_case(name)
    block = module_of(case)
    ins = [gpu(case[k]) for k in ("net", "inp", "corr", "flow")]
    with torch.no_grad():
        outs = block(*ins)
    array = solver.raft_update_block(case["net"], case["inp"], case["corr"], case["flow"], case["weights"], case["biases"])
    want = br.block_case(case)
    for o, t, a, w in zip(bc.OUTPUTS, outs, array, want):
        assert tuple(t.shape) == w.shape and t.dtype == torch.float32 and t.is_contiguous()
        got = t.cpu().numpy()
        assert np.array_equal(got, a), o                                    # the same kernels through the array path: bit for bit
        delta = float(golden[f"block/{name}/{o}_delta"])
        bar = br.bar(delta, golden[f"block/{name}/{o}_scale"])
        margins.below(f"raft block torch {name} {o}", np.abs(got - w).max(), bar)
        margins.below(f"raft block torch {name} {o} vs reference", np.abs(bc.sample_view(case, got) - golden[f"block/{name}/{o}"]).max(),
                      bar + delta)
    with torch.no_grad():
        # inputs that are not dense NCHW; the reference's `upsample` argument is ignored; the inputs are left as they were
        netp = ins[0].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        again = block(netp, *ins[1:], upsample=False)
        assert all(torch.equal(a, b) for a, b in zip(again, outs))
        assert torch.equal(ins[0], gpu(case["net"])) and torch.equal(ins[3], gpu(case["flow"]))
        # without the mask: None, and the same bits elsewhere
        net2, none, delta2 = block(*ins, compute_mask=False)
        assert none is None and torch.equal(net2, outs[0]) and torch.equal(delta2, outs[2])
        # the parts on their own: the same launches one by one
        motion = block.encoder(ins[3], ins[2])
        assert tuple(motion.shape) == (case["net"].shape[0], 128) + case["net"].shape[2:] and torch.equal(motion[:, 126:], ins[3])
        net3 = block.gru(ins[0], (ins[1], motion))
        assert torch.equal(net3, outs[0]) and torch.equal(block.flow_head(net3), outs[2])
    return block, ins, outs


def check_no_host_synchronisation(block, ins, outs):
    """Once the handle's scratch has its size a call is enqueued launches only: torch's synchronisation check stays silent, also on
    a side stream."""
    torch.cuda.synchronize(DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            again = block(*ins)
            side = torch.cuda.Stream(device=DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                third = block(*ins)
            torch.cuda.current_stream(DEV).wait_stream(side)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize(DEV)
    for a, b, c in zip(again, third, outs):
        assert torch.equal(a, c) and torch.equal(b, c)


def check_refusals(block, ins):
    net, inp, corr, flow = ins
    with torch.no_grad():
        raises(ValueError, lambda: block(net.cpu(), inp, corr, flow), "GPU")
        raises(ValueError, lambda: block(net, inp, corr.cpu(), flow), "GPU")
        raises(TypeError, lambda: block(net.double(), inp, corr, flow), "float32")
        raises(TypeError, lambda: block(net, inp, corr, flow.half()), "float32")
        raises(ValueError, lambda: block(net[:, :96], inp, corr, flow), "net must be")
        raises(ValueError, lambda: block(net, inp[:, :64], corr, flow), "inp must be")
        raises(ValueError, lambda: block(net, inp, corr[:, :196], flow), "encoder.convc1 takes 324")
        raises(ValueError, lambda: block(net, inp, corr, flow[:, :1]), "flow must be")
        raises(ValueError, lambda: block(net[:0], inp[:0], corr[:0], flow[:0]), "B H W = 0")
        raises(ValueError, lambda: block(net, inp, corr[:, :, :1], flow), "corr must be")
        raises(ValueError, lambda: BasicUpdateBlock().forward(net, inp, corr, flow), "GPU")          # parameters on the CPU
        raises(TypeError, lambda: BasicUpdateBlock().to(DEV).double().forward(net, inp, corr, flow), "float32")
        raises(ValueError, lambda: FlowHead().to(DEV)((net[:, :100], net[:, 100:])), "multiple of 32")
        raises(ValueError, lambda: BasicMotionEncoder().to(DEV)(flow, corr[:, :196]), "takes 324")
    # grad mode on: the parameters require grad
    raises(ValueError, lambda: block(net, inp, corr, flow), "forward only")
    for p in block.parameters():
        p.requires_grad_(False)
    raises(ValueError, lambda: block(net.clone().requires_grad_(True), inp, corr, flow), "forward only")
    # ... grad mode on without such a tensor is fine, and nothing above left an error on the device
    torch.cuda.synchronize(DEV)
    assert tuple(block(net, inp, corr, flow)[0].shape) == tuple(net.shape)
    torch.cuda.synchronize(DEV)


def stock_lookup(pyramid, coords, radius):
    """CorrBlock.__call__ restated with grid_sample (bilinear, align_corners, zero padding); the first window index moves x."""
    B, _, h, w = coords.shape
    r = radius
    d = torch.linspace(-r, r, 2 * r + 1, dtype=coords.dtype)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), -1).view(1, 2 * r + 1, 2 * r + 1, 2)
    out = []
    for l, corr in enumerate(pyramid):
        centroid = coords.permute(0, 2, 3, 1).reshape(B * h * w, 1, 1, 2) / 2 ** l
        at = centroid + delta
        H, W = corr.shape[-2:]
        grid = torch.stack([2 * at[..., 0] / (W - 1) - 1, 2 * at[..., 1] / (H - 1) - 1], -1)
        out.append(F.grid_sample(corr, grid, align_corners=True).view(B, h, w, -1))
    return torch.cat(out, -1).permute(0, 3, 1, 2).contiguous()


def stock_upsample(flow, mask):
    N, _, H, W = flow.shape
    mask = torch.softmax(mask.view(N, 1, 9, 8, 8, H, W), 2)
    up = F.unfold(8 * flow, [3, 3], padding=1).view(N, 2, 9, 1, 1, H, W)
    return torch.sum(mask * up, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * H, 8 * W)


def stock_loop(stock, fmap1, fmap2, net, inp, iters, dtype):
    """The refinement loop of raft/core/raft.py:86-140 after the encoders, in stock torch on the CPU at `dtype`."""
    stock = stock.to(dtype)
    fmap1, fmap2, net, inp = (t.to(dtype) for t in (fmap1, fmap2, net, inp))
    B, dim, h, w = fmap1.shape
    corr = torch.matmul(fmap1.view(B, dim, h * w).transpose(1, 2), fmap2.view(B, dim, h * w)).view(B * h * w, 1, h, w) / dim ** 0.5
    pyramid = [corr]
    for _ in range(3):
        pyramid.append(F.avg_pool2d(pyramid[-1], 2, stride=2))
    ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
    coords0 = torch.stack([xs, ys], 0)[None].repeat(B, 1, 1, 1)
    coords1 = coords0.clone()
    with torch.no_grad():
        for _ in range(iters):
            net, mask, delta = stock(net, inp, stock_lookup(pyramid, coords1, 4), coords1 - coords0)
            coords1 = coords1 + delta
            up = stock_upsample(coords1 - coords0, mask)
    return net, up


def check_refinement_loop(block_case_name="9x11", iters=2):
    """Two iterations of CorrBlock -> BasicUpdateBlock -> upsample_flow at 16 x 16 features (the smallest four-level pyramid)
    against the same loop in stock torch f64 on the CPU.  Bar: 8 x max(delta, 2^-23 scale), delta = the stock loop's own f32 error
    against its f64 self on the CPU, computed here."""
    case = bc.make_block_case(block_case_name)
    rng = np.random.default_rng(31799)
    h = w = 16
    fmap1 = torch.from_numpy(rng.normal(0, 1, (1, 256, h, w)).astype(np.float32))
    fmap2 = torch.from_numpy(rng.normal(0, 1, (1, 256, h, w)).astype(np.float32))
    net = torch.from_numpy(np.tanh(rng.normal(0, 1, (1, 128, h, w))).astype(np.float32))
    inp = torch.from_numpy(np.maximum(rng.normal(0, 1, (1, 128, h, w)), 0).astype(np.float32))
    stock = StockBlock()
    stock.load_state_dict(br.state_dict(case))
    net32, up32 = stock_loop(stock, fmap1, fmap2, net, inp, iters, torch.float32)
    net64, up64 = stock_loop(stock, fmap1, fmap2, net, inp, iters, torch.float64)

    block = module_of(case)
    with torch.no_grad():
        corr_fn = CorrBlock(fmap1.to(DEV), fmap2.to(DEV), num_levels=4, radius=4)
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=DEV), torch.arange(w, dtype=torch.float32, device=DEV),
                                indexing="ij")
        coords0 = torch.stack([xs, ys], 0)[None]
        coords1 = coords0.clone()
        n, i = net.to(DEV), inp.to(DEV)
        for _ in range(iters):
            n, mask, delta = block(n, i, corr_fn(coords1), coords1 - coords0)
            coords1 = coords1 + delta
            up = upsample_flow(coords1 - coords0, mask)
    for name, got, w32, w64 in (("net", n, net32, net64), ("flow_up", up, up32, up64)):
        delta, scale = float((w32.double() - w64).abs().max()), float(w64.abs().max())
        err = float((got.cpu().double() - w64).abs().max())
        print(f"refinement loop {name}: max |kernels - f64| {err:.3e}, the stock f32 loop's own {delta:.3e}, scale {scale:.3f}")
        margins.below(f"raft refinement loop {name}", err, br.bar(delta, scale))


if __name__ == "__main__":
    torch.cuda.init()
    golden = np.load(br.GOLDEN)
    solver = tc.solver(DEV)
    kept = None
    for name in ("5x7b3", "3x2", "9x11"):
        res = check_case(solver, golden, name)
        if name == "9x11":
            kept = res
    check_no_host_synchronisation(*kept)
    check_refusals(*kept[:2])
    check_refinement_loop()
    print("raft block torch module ok")
