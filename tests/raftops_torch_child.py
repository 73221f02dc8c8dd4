"""Child process of tests/test_gpu_raftops.py::test_torch_module (python -m tests.raftops_torch_child): torch is imported first,
then the library; robust_cvd_amd.raft_ops.CorrBlock / upsample_flow on GPU tensors against the array path
(Solver.raft_corr_pyramid / raft_corr_lookup / raft_upsample_flow) and the float64 restatement, with the bars of
tests/test_gpu_raftops.py."""
import numpy as np
import torch

from robust_cvd_amd import torch_common as tc
from robust_cvd_amd.raft_ops import CorrBlock, upsample_flow
from tests import margins
from tests import raftops_cases as rc
from tests import raftops_reference as rr

DEV = torch.device("cuda", 0)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raises(exc, call, word=None):
    try:
        call()
    except exc as e:
        assert word is None or word in str(e), (word, str(e))
    else:
        raise AssertionError(f"{exc.__name__} expected")


def check_corr(solver, golden, name):
    case = rc.make_corr_case(name)
    B, h, w, dim, levels, r = rc.CORR[name]
    f1, f2, coords = gpu(case["fmap1"]), gpu(case["fmap2"]), gpu(case["coords"])
    with torch.no_grad():
        block = CorrBlock(f1, f2, num_levels=levels, radius=r)
        out = block(coords)
        raw = torch.matmul(f1.view(B, dim, h * w).transpose(1, 2), f2.view(B, dim, h * w)).reshape(B * h * w, h, w).cpu().numpy()
    # the reference's attributes and shapes
    assert block.num_levels == levels and block.radius == r and len(block.corr_pyramid) == levels
    for l, t in enumerate(block.corr_pyramid):
        assert tuple(t.shape) == (B * h * w, 1, h >> l, w >> l) and t.dtype == torch.float32 and t.is_contiguous()
    n = 2 * r + 1
    assert tuple(out.shape) == (B, levels * n * n, h, w) and out.dtype == torch.float32 and out.is_contiguous()
    # the same kernels on the module's own matmul output through the array path: bit for bit
    pyr = solver.raft_corr_pyramid(raw, dim, levels)
    for t, a in zip(block.corr_pyramid, pyr):
        assert np.array_equal(t[:, 0].cpu().numpy(), a)
    look = solver.raft_corr_lookup(pyr, case["coords"], r)
    assert np.array_equal(out.cpu().numpy(), look)
    # ... and the bars against the float64 restatement
    pyr64 = rr.pyramid(raw, dim, levels)
    look64 = rr.lookup(pyr64, case["coords"], r)
    assert np.array_equal(pyr[0], rr.level0_f32(raw, dim))
    for l in range(1, levels):
        margins.below(f"raft torch pyramid {name} level {l}", np.abs(block.corr_pyramid[l][:, 0].cpu().numpy() - pyr64[l]).max(),
                      rr.bar(golden[name + "/delta_pyr"], golden[name + "/scale_pyr"]))
    margins.below(f"raft torch lookup {name}", np.abs(out.cpu().numpy() - look64).max(),
                  rr.bar(golden[name + "/delta_lookup"], golden[name + "/scale_lookup"]))
    # a non-contiguous coords: the same values
    wide = torch.zeros(B, 2, h, 2 * w, dtype=torch.float32, device=DEV)
    wide[..., ::2] = coords
    strided = wide[..., ::2]
    assert not strided.is_contiguous()
    with torch.no_grad():
        assert torch.equal(block(strided), out)
        # an input that requires grad is fine where no graph is recorded
        assert torch.equal(block(coords.clone().requires_grad_(True)), out)
    return block, coords, out


def check_upsample(solver, golden, name):
    case = rc.make_upsample_case(name)
    flow, mask = gpu(case["flow"]), gpu(case["mask"])
    up = upsample_flow(flow, mask)
    N, _, H, W = case["flow"].shape
    assert tuple(up.shape) == (N, 2, 8 * H, 8 * W) and up.dtype == torch.float32 and up.is_contiguous()
    assert np.array_equal(up.cpu().numpy(), solver.raft_upsample_flow(case["flow"], case["mask"]))
    margins.below(f"raft torch upsampling {name}", np.abs(up.cpu().numpy() - rr.upsample(case["flow"], case["mask"])).max(),
                  rr.bar(golden[name + "/delta"], golden[name + "/scale"]))
    # non-contiguous inputs: the same values
    perm = mask.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not perm.is_contiguous() or min(H, W) == 1
    assert torch.equal(upsample_flow(flow, perm), up)
    return flow, mask, up


def check_no_host_synchronisation(block, coords, out, flow, mask, up):
    """The per-iteration calls under stream capture: a synchronising or allocating runtime call of the library would end the
    capture with an error.  The replayed graph gives the eager results bit for bit.  The constructor (its matmul is torch's) runs
    with torch's own synchronisation check armed; its launch goes through the same enqueue function as the captured ones."""
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side), torch.no_grad():     # (warm-up on the capture's side stream, as torch asks for)
        block(coords), upsample_flow(flow, mask)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        got_out = block(coords)
        got_up = upsample_flow(flow, mask)
    got_out.zero_(), got_up.zero_()
    graph.replay()
    torch.cuda.synchronize(DEV)
    assert torch.equal(got_out, out) and torch.equal(got_up, up)
    case = rc.make_corr_case("square16")
    f1, f2 = gpu(case["fmap1"]), gpu(case["fmap2"])
    torch.cuda.synchronize(DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            again = CorrBlock(f1, f2, num_levels=4, radius=4)
            res = again(coords)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(res, out)


def check_refusals(block, coords):
    case = rc.make_corr_case("square16")
    f1, f2 = gpu(case["fmap1"]), gpu(case["fmap2"])
    up = rc.make_upsample_case("up1x1")
    flow, mask = gpu(up["flow"]), gpu(up["mask"])
    with torch.no_grad():
        raises(ValueError, lambda: CorrBlock(f1.cpu(), f2.cpu()), "GPU")
        raises(TypeError, lambda: CorrBlock(f1.double(), f2.double()), "float32")
        raises(TypeError, lambda: CorrBlock(f1.half(), f2.half()), "float32")
        raises(ValueError, lambda: CorrBlock(f1[..., :8, :8].contiguous(), f2[..., :8, :8].contiguous()), "2 x 2")
        raises(ValueError, lambda: CorrBlock(f1, f2, num_levels=5), "num_levels")
        raises(ValueError, lambda: CorrBlock(f1, f2, radius=5), "radius")
        raises(ValueError, lambda: CorrBlock(f1, f2, radius=0), "radius")
        raises(ValueError, lambda: CorrBlock(f1, f2[:, :, :8]), "alike")
        raises(ValueError, lambda: block(coords.cpu()), "GPU")
        raises(TypeError, lambda: block(coords.double()), "float32")
        raises(ValueError, lambda: block(coords[:, :, :8]), "coords must be")
        raises(ValueError, lambda: upsample_flow(flow.cpu(), mask.cpu()), "GPU")
        raises(TypeError, lambda: upsample_flow(flow.double(), mask.double()), "float32")
        raises(ValueError, lambda: upsample_flow(flow, mask[:, :575]), "mask must be")
    # grad mode on and an input that requires grad: forward only
    raises(RuntimeError, lambda: CorrBlock(f1.clone().requires_grad_(True), f2), "forward only")
    raises(RuntimeError, lambda: block(coords.clone().requires_grad_(True)), "forward only")
    raises(RuntimeError, lambda: upsample_flow(flow.clone().requires_grad_(True), mask), "forward only")
    # ... grad mode on without such an input is fine, and nothing above left an error on the device
    torch.cuda.synchronize(DEV)
    assert tuple(upsample_flow(flow, mask).shape) == (1, 2, 8, 8)
    torch.cuda.synchronize(DEV)


if __name__ == "__main__":
    torch.cuda.init()
    golden = np.load(rr.GOLDEN)
    solver = tc.solver(DEV)
    kept = None
    for name in rc.CORR:
        res = check_corr(solver, golden, name)
        if name == "square16":
            kept = res
    ups = None
    for name in rc.UPSAMPLE:
        res = check_upsample(solver, golden, name)
        if name == "up5x7":
            ups = res
    check_refusals(kept[0], kept[1])
    check_no_host_synchronisation(*kept, *ups)
    print("raft torch module ok")
