"""The workload-shaped product cases (tests/product_cases.py) are what tests/test_gpu_product_shapes.py needs them to be: item
counts in the 128-thread windows of the fast product kernel, uncut 768-constraint chunks, every chunk-edge pair present -- and
the oracle's dense J^T J on them is a usable reference (symmetric, consistent with its own frame blocks, positive diagonal)."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from robust_cvd_amd import synth
from robust_cvd_amd.ctypes_types import OptParams, XformDesc
from tests import product_cases as pc
from tests.test_gpu_huber import _state

NUM_CU = 256
ITEMS = {"items850": 850, "items1090": 1090}


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_item_lists_have_the_workload_shape(name):
    v = pc.make_case(name)
    F = v.num_frames
    assert (v.width, v.height) == (64, 40)
    counts = pc.pair_counts(v)
    undirected = {(min(a, b), max(a, b)) for a, b in counts}
    assert len(undirected) == 8 * F - 36 and len(undirected) >= 3 * NUM_CU   # the 768 chunk stays uncut on 256 CUs
    assert all(1 <= abs(a - b) <= 8 for a, b in counts)
    items = pc.expected_items(v, NUM_CU)
    assert abs(len(items) - ITEMS[name]) <= 10, len(items)
    assert max(max(n0, n1) for _, _, n0, n1 in items) == pc.LIST_CHUNK
    sizes = [n0 + n1 for _, _, n0, n1 in items]
    assert sizes == sorted(sizes, reverse=True)                              # longest first
    assert sum(n0 + n1 for _, _, n0, n1 in items) == v.num_constraints       # every constraint in exactly one item
    # most directed pairs keep 3 to 24 constraints
    n = np.diff(v.offsets)
    assert ((n >= 3) & (n <= 24)).mean() > 0.85
    # on a small device the same list IS cut: the rule restated here has both branches
    assert max(max(n0, n1) for _, _, n0, n1 in pc.expected_items(v, 4 * NUM_CU)) < pc.LIST_CHUNK

    by_pair = {}
    for fa, fb, n0, n1 in items:
        by_pair.setdefault((fa, fb), []).append((n0, n1))
    edge = {e: pc.edge_frames(e, F) for e in pc.EDGES}
    assert len(set(edge.values())) == len(pc.EDGES)                          # each edge on an undirected pair of its own
    a, b = edge["one_item_768_and_1"]
    assert (counts[(a, b)], counts[(b, a)]) == (768, 1) and by_pair[(a, b)] == [(768, 1)]
    a, b = edge["two_items_769"]
    assert counts[(a, b)] == 769 and [n0 for n0, _ in by_pair[(a, b)]] == [385, 384]
    a, b = edge["both_directions_split"]
    assert 900 <= counts[(a, b)] <= 1100 and 900 <= counts[(b, a)] <= 1100
    assert len(by_pair[(a, b)]) == 2 and all(440 <= n0 <= 560 and 440 <= n1 <= 560 for n0, n1 in by_pair[(a, b)])
    a, b = edge["reverse_absent"]
    assert 900 <= counts[(a, b)] <= 1100 and (b, a) not in counts
    assert len(by_pair[(a, b)]) == 2 and all(n1 == 0 and n0 > 256 for n0, n1 in by_pair[(a, b)])
    a, b = edge["long_backward_5_forward"]
    assert counts[(a, b)] == 5 and 900 <= counts[(b, a)] <= 1100
    assert sorted(n0 for n0, _ in by_pair[(a, b)]) == [2, 3] and all(n1 > 256 for _, n1 in by_pair[(a, b)])


def test_thread_rule_windows_on_256_cus():
    """The 128-thread windows of launchMatvec on 256 CUs: (1024, 2048] for SPEC 1 / 2 with KD <= 4, (768, 1536] for SPEC 1 / 2
    with KD = 16, (512, 1024] for SPEC 0 -- and which side of them the two cases' item counts fall on."""
    for kd, spec, lo, hi in ((1, 1, 1024, 2048), (4, 2, 1024, 2048), (16, 1, 768, 1536), (16, 2, 768, 1536),
                             (1, 0, 512, 1024), (4, 0, 512, 1024), (16, 0, 512, 1024)):
        block = 7 + {1: 1, 4: 12, 16: 16}[kd]
        assert pc.expected_threads(kd, spec, block, NUM_CU, lo) == 256
        assert pc.expected_threads(kd, spec, block, NUM_CU, lo + 1) == 128
        assert pc.expected_threads(kd, spec, block, NUM_CU, hi) == 128
        assert pc.expected_threads(kd, spec, block, NUM_CU, hi + 1) == 256
    # a frame block so large that a CU's LDS holds fewer 128-thread workgroups than twice its 256-thread slots
    assert pc.expected_threads(4, 1, 400, NUM_CU, 1800) == 256 and pc.expected_threads(4, 1, 19, NUM_CU, 1800) == 128


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_oracle_hfull_is_a_usable_reference(name):
    v = pc.make_case(name)
    F = v.num_frames
    o = Oracle()
    synth.load_into(o, v)
    o.reset_depth_xforms(XformDesc.grid_depth(4, 3))
    o.reset_spatial_xforms(XformDesc.spatial())
    pose, dx, _ = _state(o, F, np.random.default_rng(17))
    o.set_xform_params(dx)
    p = OptParams.defaults()
    p.num_threads = 8
    r = o.evaluate(p, 0.1, pose, want_hdiag=True, want_hfull=True)
    H, B = r["hfull"], o.block_size()
    assert H.shape == (F * B, F * B) and B == 7 + 12
    assert r["num_residual_blocks"] >= v.num_constraints * 0.95
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    blocks = np.stack([H[f * B:(f + 1) * B, f * B:(f + 1) * B] for f in range(F)])
    assert np.abs(blocks - r["hdiag"]).max() <= 1e-12 * np.abs(r["hdiag"]).max()
    assert np.diag(H).min() > 0.0          # the Jacobi-scaled metric of the GPU test divides by sqrt(H_ii H_jj)
    # the long pairs' cross blocks are there (and the absent direction's pair still couples its two frames)
    for e in pc.EDGES:
        a, b = pc.edge_frames(e, F)
        assert np.abs(H[a * B:(a + 1) * B, b * B:(b + 1) * B]).max() > 0.0
