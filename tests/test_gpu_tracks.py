"""GPU feature tracks (robust_cvd_amd/csrc/cvd_tracks.h, cvd_compute_tracks) against the numpy restatement
tests/tracks_reference.py of DepthVideoProcessor::computeTracks (reference lib/Processor.cpp:646-886): same ids, frames and
location bits, given the same corner and dynamic-distance arrays."""
import numpy as np
import pytest

from robust_cvd_amd import synth
from tests.tracks_reference import F32, compute_tracks, from_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    from robust_cvd_amd import api
    return api.Solver(0)


def _scene(F, W, H, seed, dyn=None, ties=False):
    pairs = np.array([(f, f + 1) for f in range(F - 1)], np.int32)
    v = synth.make_video(F, W, H, seed=seed, pairs=pairs)
    flow, mask = synth.make_dense_flows(v, seed=seed + 1, invalid_fraction=0.05)
    rng = np.random.default_rng(seed + 2)
    corner = rng.uniform(0, 1, (F, H, W)).astype(np.float32)
    if ties:
        corner = (np.round(corner * 8) / 8).astype(np.float32)
    dd = rng.uniform(0, 12, (F,) + dyn).astype(np.float32) if dyn else None
    return v, corner, flow, mask, dd


def _both(solver, v, corner, flow, mask, dd, active=None, first=None, last=None, present=None, **kw):
    F, W, H = v.num_frames, v.width, v.height
    active = np.ones(F, np.uint8) if active is None else np.asarray(active, np.uint8)
    first = int(np.flatnonzero(active)[0]) if first is None else first
    last = int(np.flatnonzero(active)[-1]) if last is None else last
    present = np.full(F - 1, 3, np.uint8) if present is None else present
    p = dict(spawn=20, prune=5, min_dyn=3, min_len=4)
    p.update(kw)
    ref = compute_tracks(corner, W, H, v.inv_aspect, active, first, last, flow, mask, present, dd, **p)
    out = solver.compute_tracks(corner, v.inv_aspect, active, first, last, flow, mask, present, dd,
                                spawn_distance=p["spawn"], prune_distance=p["prune"], min_dynamic_distance=p["min_dyn"],
                                min_track_length=p["min_len"])
    return ref, out, from_arrays(F, *out)


@pytest.mark.parametrize("case", [
    dict(F=12, W=96, H=56, dyn=None, ties=False, kw={}),
    dict(F=10, W=96, H=56, dyn=(28, 48), ties=True, kw={}),                       # dynamic masks at half resolution
    dict(F=10, W=80, H=48, dyn=(61, 97), ties=False, kw=dict(min_dyn=5)),          # ... and at a larger one
    dict(F=9, W=64, H=40, dyn=None, ties=True, kw=dict(spawn=4, prune=2, min_len=2)),
    dict(F=8, W=64, H=40, dyn=None, ties=False, kw=dict(spawn=0, prune=0, min_len=6)),
])
def test_tracks_match_restatement(solver, case):
    v, corner, flow, mask, dd = _scene(case["F"], case["W"], case["H"], seed=case["W"] + case["F"], dyn=case["dyn"],
                                       ties=case["ties"])
    ref, out, got = _both(solver, v, corner, flow, mask, dd, **case["kw"])
    assert len(ref.tracks) == len(got.tracks) > 0
    assert got == ref   # ids, start frames, lengths, holes, location bits
    assert sum(t is not None for t in ref.tracks) > 0


def test_tracks_range_gaps_and_missing_pairs(solver):
    F, W, H = 10, 64, 40
    v, corner, flow, mask, dd = _scene(F, W, H, seed=5, dyn=(40, 64))
    active = np.array([0, 1, 1, 1, 0, 1, 1, 1, 1, 0], np.uint8)
    present = np.array([3, 3, 1, 3, 3, 2, 3, 0, 3], np.uint8)
    ref, _, got = _both(solver, v, corner, flow, mask, dd, active=active, first=1, last=8, present=present, min_len=2)
    assert got == ref and len(ref.tracks) > 0


def test_tracks_two_runs_bitwise_equal(solver):
    v, corner, flow, mask, dd = _scene(8, 96, 56, seed=11, dyn=(56, 96), ties=True)
    args = (corner, v.inv_aspect, np.ones(8, np.uint8), 0, 7, flow, mask, np.full(7, 3, np.uint8), dd)
    a, b = solver.compute_tracks(*args), solver.compute_tracks(*args)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def test_tracks_invariants_at_full_size(solver):
    """384 x 224, defaults: continued targets of a frame lie outside each other's prune disks, spawned pixels outside the
    spawn disks stamped before them, and every kept track has at least minTrackLength observations."""
    F, W, H = 6, 384, 224
    v, corner, flow, mask, _ = _scene(F, W, H, seed=21)
    args = (corner, v.inv_aspect, np.ones(F, np.uint8), 0, F - 1, flow, mask, np.full(F - 1, 3, np.uint8), None)
    start, length, kept, off, loc = solver.compute_tracks(*args, min_track_length=1)
    assert kept.all() and len(start) > 100
    ia = F32(v.inv_aspect)
    per_frame = {f: [] for f in range(F)}
    for t in range(len(start)):
        for k in range(length[t]):
            x, y = loc[off[t] + k]
            if k == 0:   # the spawn pixel: the stored position read back
                p = (int(F32(x) * F32(W)), int(F32(y) / ia * F32(H)))
            else:        # the continued target: int(fx1 + 0.5)
                p = (int(F32(x) * F32(W) + F32(0.5)), int(F32(y) / ia * F32(H) + F32(0.5)))
            per_frame[start[t] + k].append((p, k == 0))
    for f, obs in per_frame.items():
        cont = np.array([p for p, s in obs if not s]).reshape(-1, 2)
        if len(cont) > 1:
            d2 = ((cont[:, None] - cont[None]) ** 2).sum(-1)
            np.fill_diagonal(d2, 10 ** 9)
            assert d2.min() > 5 * 5
        stamped = [tuple(p) for p in cont]
        for p in [p for p, s in obs if s]:
            assert all((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 > 20 * 20 for q in stamped)
            stamped.append(p)
    _, length4, kept4, _, _ = solver.compute_tracks(*args)
    assert np.array_equal(length4, length) and np.array_equal(kept4, length >= 4) and not kept4.all()


def test_tracks_argument_checks(solver):
    v, corner, flow, mask, _ = _scene(4, 32, 24, seed=2)
    ones = np.ones(4, np.uint8)
    pp = np.full(3, 3, np.uint8)
    with pytest.raises(RuntimeError, match=r"trackSpawnDistance must lie in \[0, 16384\] \(got -1\)"):
        solver.compute_tracks(corner, v.inv_aspect, ones, 0, 3, flow, mask, pp, None, spawn_distance=-1)
    with pytest.raises(RuntimeError, match=r"trackPruneDistance .* \(got 20000\)"):
        solver.compute_tracks(corner, v.inv_aspect, ones, 0, 3, flow, mask, pp, None, prune_distance=20000)
    with pytest.raises(RuntimeError, match=r"frame range \[2, 5\] outside \[0, 4\)"):
        solver.compute_tracks(corner, v.inv_aspect, ones, 2, 5, flow, mask, pp, None)
    with pytest.raises(RuntimeError, match="inv_aspect must be finite"):
        solver.compute_tracks(corner, 0.0, ones, 0, 3, flow, mask, pp, None)
    with pytest.raises(RuntimeError, match="null flow or mask"):
        solver.compute_tracks(corner, v.inv_aspect, ones, 0, 3, None, None, pp, None)
    # the two LDS bitmasks of a 1024 x 720 image (2 x 92160 B) exceed the LDS budget: refused before any work
    big = np.zeros((1, 720, 1024), np.float32)
    with pytest.raises(RuntimeError, match=r"image too large: .* 1024 x 720 image need 184320 B"):
        solver.compute_tracks(big, 0.7, np.ones(1, np.uint8), 0, 0)
