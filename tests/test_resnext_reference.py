"""The float64 restatement of the ResNeXt backbone (tests/resnext_reference.py) against the fixture minted from stock torch modules
(tests/golden/reference_py/resnext_golden.npz) and, where torchvision is importable, against its own ResNet(Bottleneck, ...); the
conditions on the seeded inputs; the convolution table, the state-dict keys and the split rule of the package against the lists
written out in tests/resnext_cases.py; the shape checks.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from robust_cvd_amd import api
from tests import midas_cases as mc
from tests import resnext_cases as rc
from tests import resnext_reference as rr
from tests.codegen_util import ROOT

FAMILIES = (("grouped", rc.GROUPED_CASES, rc.make_grouped_case, rr.grouped_case), ("conv", rc.CONV_CASES, rc.make_conv_case, rr.conv_case),
            ("pool", rc.POOL_CASES, rc.make_pool_case, lambda c: rr.maxpool(c["x"])), ("block", rc.BLOCK_CASES, rc.make_block_case, rr.block_case),
            ("net", rc.NET_CASES, rc.make_net_case, rr.net_case))


@pytest.fixture(scope="module")
def golden():
    return np.load(rr.GOLDEN)


@pytest.fixture(scope="module")
def backbones():
    """Per backbone case: (case, the four f64 feature maps): computed once, shared."""
    out = {}
    for name in rc.BACKBONE_CASES:
        case = rc.make_backbone_case(name)
        out[name] = (case, rr.backbone_case(case))
    return out


def within_delta(golden, key, case, want, samples):
    assert rc.input_digest(case) == golden[f"{key}/input_sha256"].tobytes().decode(), "the seeded case drifted from the minted one"
    delta, scale = float(golden[f"{key}/out_delta"]), float(golden[f"{key}/out_scale"])
    assert np.abs(want).max() == pytest.approx(scale, rel=1e-12)
    assert delta <= 64 * rr.EPS32 * max(scale, 1.0), "torch's f32 arithmetic lies far from the restatement"
    assert np.abs(rc.sample_view(want, samples) - golden[f"{key}/out"]).max() <= delta


@pytest.mark.parametrize("family,name", [(f[0], n) for f in FAMILIES for n in f[1]])
def test_restatement_lies_within_delta_of_stock_torch(golden, family, name):
    make, restate = dict((f[0], (f[2], f[3])) for f in FAMILIES)[family]
    case = make(name)
    within_delta(golden, f"{family}/{name}", case, restate(case), case["samples"])
    if name.startswith("planted"):
        assert float(golden[f"{family}/{name}/out_delta"]) == 0.0          # exact in any arithmetic


@pytest.mark.parametrize("name", list(rc.BACKBONE_CASES))
def test_backbone_restatement_and_the_conditions_on_its_maps(golden, backbones, name):
    case, maps = backbones[name]
    rr.check_conditions(name, maps)
    for k in range(4):
        within_delta(golden, f"backbone/{name}/map{k + 1}", case, maps[k], case["samples"][k])


def test_the_seeded_parameters_have_the_stated_distributions():
    rng = np.random.default_rng(5)
    for shape in ((64, 3, 7, 7), (256, 8, 3, 3), (512, 2048, 1, 1)):
        w = rc.he_weight(rng, shape)
        bound = np.sqrt(6.0 / (shape[1] * shape[2] * shape[3]))
        assert w.dtype == np.float32 and np.abs(w).max() <= bound and np.abs(w).max() > 0.9 * bound
        assert w.var() == pytest.approx(bound ** 2 / 3, rel=0.2)
    case = rc.make_backbone_case("small_32x32")
    table = rc.conv_table(case["blocks"], case["groups"], case["width_per_group"])
    assert len(table) == len(case["params"])
    for (_c, _n, _k, _nk, shape, _s, _g, last), (w, (gamma, beta, mean, var)) in zip(table, case["params"]):
        assert w.shape == shape and np.abs(w).max() <= np.sqrt(6.0 / (shape[1] * shape[2] * shape[3]))
        lo, hi = (0.2, 0.5) if last else (0.5, 1.5)
        assert lo <= gamma.min() and gamma.max() <= hi and 0.5 <= var.min() and var.max() <= 1.5
        assert np.abs(beta).max() < 0.6 and np.abs(mean).max() < 0.6
    assert sum(1 for t in table if t[7]) == sum(case["blocks"])


def test_the_conv_table_and_the_keys_of_the_real_network():
    blocks, groups, wpg = rc.REAL
    table = rc.conv_table(blocks, groups, wpg)
    mine = api.resnext_conv_table(blocks, groups, wpg)
    assert len(table) == len(mine) == 104
    for (conv, norm, key, norm_key, shape, stride, g, _last), c in zip(table, mine):
        assert (c.name, c.norm, c.key, c.norm_key, c.weight_shape, c.stride, c.groups) == (conv, norm, key, norm_key, shape, stride, g)
        assert (c.out_channels, c.kernel_size) == (shape[0], shape[2]) and c.in_channels == shape[1] * g
    keys = rc.state_dict_keys(blocks, groups, wpg)
    assert len(keys) == 624 and [k for k, _ in keys] == api.resnext_state_dict_keys()
    assert keys[0] == ("pretrained.layer1.0.weight", (64, 3, 7, 7)) and keys[5][0] == "pretrained.layer1.1.num_batches_tracked"
    assert keys[6] == ("pretrained.layer1.4.0.conv1.weight", (256, 64, 1, 1)) and keys[12][1] == (256, 8, 3, 3)
    assert keys[-6] == ("pretrained.layer4.2.conv3.weight", (2048, 2048, 1, 1))
    assert [s for k, s in keys if k.endswith("layer4.0.conv2.weight")] == [(2048, 64, 3, 3)]
    assert ("pretrained.layer4.0.downsample.1.running_var", (2048,)) in keys
    assert [c.weight_shape[1] for c in api.resnext_conv_table(*rc.SMALL) if c.groups > 1] == [8, 8, 16, 32, 32, 64]


def test_the_torch_modules_have_the_reference_checkpoints_keys():
    """MidasNet(backbone=resnext101_32x8d()): 624 pretrained.* keys and the 42 scratch.* keys in the reference's order and shapes
    (on the meta device: no memory, no initialisation)."""
    import torch
    from robust_cvd_amd import midas
    with torch.device("meta"):
        net = midas.midas_v21()
        small = midas.ResNeXt(*rc.SMALL)
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert got[:624] == rc.state_dict_keys(*rc.REAL)
    assert tuple(k for k, _ in got[624:]) == mc.STATE_DICT_KEYS and len(got) == 666
    assert [("pretrained." + k, tuple(v.shape)) for k, v in small.state_dict().items()] == rc.state_dict_keys(*rc.SMALL)
    assert isinstance(net.pretrained, midas.ResNeXt) and net.pretrained.out_channels == (256, 512, 1024, 2048)
    assert all(callable(getattr(net.pretrained, f"layer{k}")) for k in (1, 2, 3, 4))


def test_stock_torch_modules_have_the_same_keys_and_torchvision_agrees_where_installed():
    import torch
    case = rc.make_backbone_case("small_32x32")
    stock = rr.stock_backbone(case)
    assert [("pretrained." + k, tuple(v.shape)) for k, v in stock.state_dict().items()] == rc.state_dict_keys(*rc.SMALL)
    tv = pytest.importorskip("torchvision.models.resnet")
    net = tv.ResNet(tv.Bottleneck, list(case["blocks"]), groups=case["groups"], width_per_group=case["width_per_group"])
    mine = rr.stock_resnet(case["blocks"], case["groups"], case["width_per_group"])
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items() if not k.startswith("fc.")] == \
        [(k, tuple(v.shape)) for k, v in mine.state_dict().items()]
    rr.load_parameters(mine, case["params"], case["blocks"], case["groups"], case["width_per_group"])
    net.load_state_dict(dict(mine.state_dict(), **{"fc.weight": net.fc.weight, "fc.bias": net.fc.bias}), strict=True)
    for a, b in zip(rr.stock_maps(rr.midas_backbone(net).eval(), case["images"]), rr.stock_maps(stock, case["images"])):
        assert torch.equal(a, b)


def test_the_split_rule():
    """api.resnext_split is the twin of rxSplit in csrc/cvd_resnext.h: a function of K and the output pixels of one image alone."""
    for name, want in rc.EXPECTED_SPLIT.items():
        cin, _cout, k, stride, (_B, H, W), _form = rc.CONV_CASES[name]
        assert api.resnext_split(cin * k * k, rc.out_size(H, stride) * rc.out_size(W, stride), k) == want, name
    # 384 x 224 frames: layer3 is 24 x 14 = 336 pixels, layer4 12 x 7 = 84
    assert [api.resnext_split(K, 336) for K in (512, 1024)] == [2, 4] and [api.resnext_split(K, 84) for K in (1024, 2048)] == [4, 8]
    assert api.resnext_split(256, 96 * 56) == 1 and api.resnext_split(147, 192 * 112, 7) == 1
    for K in (32, 256, 257, 2048, 8192, 100000):
        for hw in (1, 64, 65, 336, 4096, 10 ** 6):
            S = api.resnext_split(K, hw)
            chains = ((K + 31) // 32 + 7) // 8
            assert 1 <= S <= min(api.RESNEXT_MAX_SPLIT, chains)
            per = (chains + S - 1) // S
            assert (S - 1) * per < chains                  # no empty slice
    text = open(os.path.join(ROOT, "robust_cvd_amd", "csrc", "cvd_resnext.h")).read()
    assert re.search(r"constexpr int kRxMaxSplit = 32;", text) and re.search(r"kFold = KS == 1 \? 8 : 3;", text)
    assert re.search(r"kChunkChannels = KS == 1 \? 32 : 2;", text) and "long long want = 64 / tiles;" in text


def test_shape_checks_refuse_before_any_device_work():
    norm = [(256,)] * 4
    assert api.resnext_check_grouped_conv((2, 256, 5, 7), (256, 8, 3, 3), 2, norm) == (2, 5, 7, 32, 8, 3, 4)
    with pytest.raises(ValueError, match=r"one of \(8, 16, 32, 64\) \(got 12\)"):
        api.resnext_check_grouped_conv((1, 48, 5, 7), (48, 12, 3, 3))
    with pytest.raises(ValueError, match="no whole groups"):
        api.resnext_check_grouped_conv((1, 40, 5, 7), (40, 16, 3, 3))
    with pytest.raises(ValueError, match="in and out channels are equal"):
        api.resnext_check_grouped_conv((1, 64, 5, 7), (32, 8, 3, 3))
    with pytest.raises(ValueError, match="3 x 3"):
        api.resnext_check_grouped_conv((1, 64, 5, 7), (64, 8, 1, 1))
    with pytest.raises(ValueError, match="stride must be 1 or 2"):
        api.resnext_check_grouped_conv((1, 64, 5, 7), (64, 8, 3, 3), 3)
    with pytest.raises(ValueError, match="four vectors"):
        api.resnext_check_grouped_conv((1, 64, 5, 7), (64, 8, 3, 3), 1, [(64,)] * 3)
    with pytest.raises(ValueError, match="eps must be > 0"):
        api.resnext_check_grouped_conv((1, 64, 5, 7), (64, 8, 3, 3), 1, [(64,)] * 4, 0.0)
    assert api.resnext_check_conv((2, 40, 5, 7), (70, 40, 1, 1), 2, [(70,)] * 4, 1e-5, (2, 70, 3, 4)) == (2, 5, 7, 40, 70, 1, 3, 4)
    assert api.resnext_check_conv((1, 3, 9, 11), (64, 3, 7, 7), 2)[-2:] == (5, 6)
    for weight, stride in (((64, 3, 7, 7), 1), ((64, 3, 3, 3), 1), ((64, 3, 5, 5), 2)):
        with pytest.raises(ValueError, match="kernel_size, stride"):
            api.resnext_check_conv((1, 3, 9, 11), weight, stride)
    with pytest.raises(ValueError, match="takes 41"):
        api.resnext_check_conv((1, 40, 5, 7), (70, 41, 1, 1))
    with pytest.raises(ValueError, match="residual must be"):
        api.resnext_check_conv((2, 40, 5, 7), (70, 40, 1, 1), 2, None, 1e-5, (2, 70, 5, 7))
    with pytest.raises(ValueError, match="split must be 0"):
        api.resnext_check_conv((2, 40, 5, 7), (70, 40, 1, 1), split=3)
    assert api.resnext_check_maxpool((2, 3, 7, 9)) == (2, 3, 7, 9, 4, 5) and api.resnext_check_maxpool((1, 1, 1, 1))[-2:] == (1, 1)
    with pytest.raises(ValueError, match="= 0"):
        api.resnext_check_maxpool((1, 0, 4, 4))
    table = api.resnext_conv_table(*rc.SMALL)
    shapes, norms = [c.weight_shape for c in table], [[(c.out_channels,)] * 4 for c in table]
    B, H, W, _table, outs = api.resnext_check_backbone((2, 3, 64, 96), *rc.SMALL, shapes, norms)
    assert (B, H, W) == (2, 64, 96) and outs == [(2, 256, 16, 24), (2, 512, 8, 12), (2, 1024, 4, 6), (2, 2048, 2, 3)]
    with pytest.raises(ValueError, match="multiples of 32"):
        api.resnext_check_backbone((2, 3, 64, 90), *rc.SMALL, shapes, norms)
    with pytest.raises(ValueError, match="4 channels per group"):
        api.resnext_check_backbone((2, 3, 64, 96), (2, 1, 2, 1), 4, 4, shapes, norms)
    with pytest.raises(ValueError, match=r"layer2.0.conv2.weight must be"):
        api.resnext_check_backbone((2, 3, 64, 96), *rc.SMALL, shapes[:9] + [(64, 8, 3, 3)] + shapes[10:], norms)
    with pytest.raises(ValueError, match="eps must be > 0"):
        api.resnext_check_backbone((2, 3, 64, 96), *rc.SMALL, shapes, norms, eps=-1.0)
    with pytest.raises(ValueError, match="weights and norms are expected"):
        api.resnext_check_backbone((2, 3, 64, 96), *rc.SMALL, shapes[:-1], norms)
    with pytest.raises(ValueError, match="blocks must be four counts"):
        api.resnext_conv_table((3, 4, 0, 3), 32, 8)


def test_the_entry_points_are_declared_exported_and_documented():
    names = ["cvd_resnext_grouped_conv_device", "cvd_resnext_conv_device", "cvd_resnext_maxpool_device", "cvd_midas_backbone_device",
             "cvd_midas_backbone_timed"]
    header = open(os.path.join(ROOT, "include", "cvd_hip.h")).read()
    lib = C.CDLL(api.load_library()._name)
    for name in names:
        assert name in api.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert re.search(r"\*/\nint32_t " + name + r"\(cvd_handle\* h,", header), name          # a documented declaration
    # the header map of the front-end operators' kernel headers is the head of the one unit that includes them
    unit = open(os.path.join(ROOT, "robust_cvd_amd", "csrc", "cvd_frontend.hip")).read()
    assert "cvd_resnext.h: k_rx_gconv, k_rx_conv, k_rx_fold, k_rx_maxpool" in unit[:unit.index("#include")]


def test_nothing_names_the_hub():
    """Nothing in the package or the tools fetches: the string `torch.hub` appears nowhere in them."""
    word = "torch" + ".hub"
    for top in ("robust_cvd_amd", "tools"):
        for folder, _dirs, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".h", ".hip", ".cpp", ".sh")):
                    assert word not in open(os.path.join(folder, f), errors="replace").read(), os.path.join(folder, f)
