"""Child process of tests/test_gpu_raftgru.py::test_torch_module (python -m tests.raftgru_torch_child): torch is imported first,
then the library; robust_cvd_amd.raft_ops.SepConvGRU on GPU tensors against the array path (Solver.raft_sepconv_gru), the float64
restatement and the reference's stored values, with the bars of tests/test_gpu_raftgru.py."""
import io

import numpy as np
import torch

from robust_cvd_amd import torch_common as tc
from robust_cvd_amd.raft_ops import SepConvGRU
from tests import margins
from tests import raftgru_cases as gc
from tests import raftgru_reference as gr

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


class StockGRU(torch.nn.Module):
    """A stock-torch module of the reference's layout (its parameter names and shapes), for the state dict round trip."""

    def __init__(self):
        super().__init__()
        for name in gc.PARAMETERS:
            k = gc.weight_shape(name)[2:]
            setattr(self, name, torch.nn.Conv2d(gc.HIDDEN + gc.INPUT, gc.HIDDEN, k, padding=(k[0] // 2, k[1] // 2)))


def module_of(case):
    """The drop-in with the case's parameters, loaded through a state dict SAVED from a stock-torch module of the same layout."""
    stock = StockGRU()
    stock.load_state_dict(gr.state_dict(case))
    buf = io.BytesIO()
    torch.save(stock.state_dict(), buf)
    buf.seek(0)
    gru = SepConvGRU(hidden_dim=128, input_dim=256)
    result = gru.load_state_dict(torch.load(buf), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    return gru.to(DEV)


def check_case(solver, golden, name):
    case = gc.make_case(name)
    gru = module_of(case)
    h, x = gpu(case["h"]), gpu(case["x"])
    with torch.no_grad():
        out = gru(h, x)
    assert tuple(out.shape) == case["h"].shape and out.dtype == torch.float32 and out.is_contiguous()
    assert out.data_ptr() != h.data_ptr()
    got = out.cpu().numpy()
    # the same kernels through the array path: bit for bit
    assert np.array_equal(got, solver.raft_sepconv_gru(case["h"], case["x"], case["weights"], case["biases"]))
    delta = float(golden[name + "/delta"])
    bar = gr.bar(delta, golden[name + "/scale"])
    want = gr.sepconv_gru(case["h"], case["x"], case["weights"], case["biases"])
    margins.below(f"raft gru torch {name}", np.abs(got - want).max(), bar)
    margins.below(f"raft gru torch {name} vs reference", np.abs(gc.sample_view(case, got) - golden[name + "/out"]).max(), bar + delta)
    with torch.no_grad():
        # the segment form: views of x are made contiguous by the module, the bits stay
        assert torch.equal(gru(h, (x[:, :128], x[:, 128:])), out)
        assert torch.equal(gru(h, (x[:, :32].contiguous(), x[:, 32:128].contiguous(), x[:, 128:].contiguous())), out)
        # inputs that are not dense NCHW
        hp = h.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert torch.equal(gru(hp, x), out)
        # the input is left as it was, and a second call repeats the bits
        assert torch.equal(h, gpu(case["h"])) and torch.equal(gru(h, x), out)
    return gru, h, x, out


def check_refusals(gru, h, x):
    with torch.no_grad():
        raises(ValueError, lambda: SepConvGRU(hidden_dim=96, input_dim=256), "hidden_dim")
        raises(ValueError, lambda: SepConvGRU(hidden_dim=128, input_dim=320), "input_dim")
        raises(ValueError, lambda: gru(h.cpu(), x), "GPU")
        raises(ValueError, lambda: gru(h, x.cpu()), "GPU")
        raises(TypeError, lambda: gru(h.double(), x), "float32")
        raises(TypeError, lambda: gru(h, x.half()), "float32")
        raises(ValueError, lambda: gru(h[:, :96], x), "hidden_dim")
        raises(ValueError, lambda: gru(h, x[:, :192]), "input_dim")
        raises(ValueError, lambda: gru(h, (x[:, :100], x[:, 100:])), "multiple of 32")
        raises(ValueError, lambda: gru(h, (x[:, :64],) * 4), "up to 3")
        raises(ValueError, lambda: gru(h[:0], x[:0]), "B H W = 0")
        raises(ValueError, lambda: gru(h, x[:, :, :1]), "segment of x")
        raises(ValueError, lambda: SepConvGRU().forward(h, x), "GPU")          # parameters on the CPU
        raises(TypeError, lambda: SepConvGRU().to(DEV).double().forward(h, x), "float32")
    # grad mode on: the parameters require grad
    raises(ValueError, lambda: gru(h, x), "forward only")
    for p in gru.parameters():
        p.requires_grad_(False)
    raises(ValueError, lambda: gru(h.clone().requires_grad_(True), x), "forward only")
    raises(ValueError, lambda: gru(h, (x[:, :128], x[:, 128:].clone().requires_grad_(True))), "forward only")
    # ... grad mode on without such a tensor is fine, and nothing above left an error on the device
    torch.cuda.synchronize(DEV)
    assert tuple(gru(h, x).shape) == tuple(h.shape)
    torch.cuda.synchronize(DEV)


def check_no_host_synchronisation(gru, h, x, out):
    """Once the handle's scratch has its size a call is four enqueued launches: torch's synchronisation check stays silent, also on
    a side stream."""
    torch.cuda.synchronize(DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            again = gru(h, x)
            side = torch.cuda.Stream(device=DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                third = gru(h, x)
            torch.cuda.current_stream(DEV).wait_stream(side)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize(DEV)
    assert torch.equal(again, out) and torch.equal(third, out)


if __name__ == "__main__":
    torch.cuda.init()
    golden = np.load(gr.GOLDEN)
    solver = tc.solver(DEV)
    kept = None
    for name in gc.CASES:
        res = check_case(solver, golden, name)
        if name == "9x11":
            kept = res
    check_no_host_synchronisation(*kept)
    check_refusals(*kept[:3])
    print("raft gru torch module ok")
