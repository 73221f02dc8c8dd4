"""Known answers of the computeTracks restatement (tests/tracks_reference.py, reference lib/Processor.cpp:646-886) and of the
track table's file format (lib/core/TrackTable-impl.h).  CPU only."""
import struct

import numpy as np
import pytest

from tests.tracks_reference import F32, Table, compute_tracks, deserialize, import_tracks_csv, serialize


def _ia(W, H):
    return F32(1.0) / (F32(W) / F32(H))


def _case(F, W, H, flow=(0.0, 0.0), dyn_points=None, corner_points=None, mask=255, present=3):
    """Constant flow and mask per pair; dyn: 0 everywhere but the listed {frame: [(x, y, value)]} (None: no dyn map)."""
    corner = np.zeros((F, H, W), np.float32)
    for f, pts in (corner_points or {}).items():
        for x, y, v in pts:
            corner[f, y, x] = v
    fl = np.zeros((F - 1, H, W, 2), np.float32)
    fl[..., 0], fl[..., 1] = flow
    mk = np.full((F - 1, H, W), mask, np.uint8)
    dyn = None
    if dyn_points is not None:
        dyn = np.zeros((F, H, W), np.float32)
        for f, pts in dyn_points.items():
            if pts == "all":
                dyn[f] = 10.0
                continue
            for x, y, v in pts:
                dyn[f, y, x] = v
    return corner, fl, mk, np.full(F - 1, present, np.uint8), dyn


def _run(case, W, H, active=None, first=0, last=None, **kw):
    corner, fl, mk, pp, dyn = case
    F = corner.shape[0]
    active = np.ones(F, np.uint8) if active is None else np.asarray(active, np.uint8)
    last = F - 1 if last is None else last
    return compute_tracks(corner, W, H, _ia(W, H), active, first, last, fl, mk, pp, dyn, **kw)


def test_one_corner_carried_by_constant_flow():
    F, W, H = 5, 32, 24
    case = _case(F, W, H, flow=(2.0, 1.0), corner_points={0: [(10, 8, 1.0)]})
    t = _run(case, W, H, spawn=100, min_len=1)
    assert len(t.tracks) == 1 and t.tracks[0][0] == 0
    locs = t.tracks[0][1]
    assert locs.shape == (F, 2)
    ia = _ia(W, H)
    px = locs[:, 0] * W
    py = locs[:, 1] / ia * H
    assert np.allclose(px, 10 + 2 * np.arange(F), atol=1e-4) and np.allclose(py, 8 + np.arange(F), atol=1e-4)
    assert t.frame_tracks(3) == [0]


@pytest.mark.parametrize("a_first", [True, False])
def test_prune_disk_lower_id_wins(a_first):
    """A = (5, 10) and B = (12, 10) spawn in frame 0 (dyn map: the only candidates); A moves +4, B -1: the targets (9, 10) and
    (11, 10) lie 2 px apart (<= trackPruneDistance 5), so the track with the lower id (the higher corner response) wins."""
    F, W, H = 2, 32, 32
    ca, cb = (2.0, 1.0) if a_first else (1.0, 2.0)
    case = _case(F, W, H, corner_points={0: [(5, 10, ca), (12, 10, cb)]}, dyn_points={0: [(5, 10, 9.0), (12, 10, 9.0)], 1: "all"})
    fl = case[1]
    fl[0, 10, 5] = (4.0, 0.0)
    fl[0, 10, 12] = (-1.0, 0.0)
    t = _run(case, W, H, spawn=3, min_len=1)
    assert len(t.tracks) == 2
    lens = [len(tr[1]) for tr in t.tracks]
    assert lens == [2, 1]
    winner = t.tracks[0][1][1] * np.array([W, H / _ia(W, H)])
    assert np.allclose(winner, (9, 10) if a_first else (11, 10), atol=1e-4)
    # pruning by length leaves the loser's id behind as a hole
    t2 = _run(case, W, H, spawn=3, min_len=2)
    assert len(t2.tracks) == 2 and t2.has_track(0) and not t2.has_track(1) and t2.tracks[1] is None
    assert serialize(t2)[8 + 1 + 16 + 16:][:1] == b"\x00"


def test_spawn_disk_seeded_by_continued_tracks():
    """Frame 1: the continued track at (10, 10) stamps its spawn disk first, so the strongest candidate (12, 10) is refused and
    (20, 10) spawns as track 1."""
    F, W, H = 3, 32, 32
    case = _case(F, W, H, corner_points={0: [(10, 10, 5.0)], 1: [(12, 10, 9.0), (20, 10, 1.0)]},
                 dyn_points={0: [(10, 10, 9.0)], 1: [(10, 10, 9.0), (12, 10, 9.0), (20, 10, 9.0)], 2: "all"})
    t = _run(case, W, H, spawn=4, min_len=1)
    assert [tr[0] for tr in t.tracks] == [0, 1]
    assert np.allclose(t.tracks[1][1][0, 0] * W, 20)
    assert t.frame_tracks(1) == [0, 1] and t.frame_tracks(2) == [0, 1]


def test_negative_truncation_lands_on_column_zero():
    F, W, H = 2, 16, 16
    for dx, kept in ((-1.2, True), (-1.6, False)):
        case = _case(F, W, H, flow=(dx, 0.0), corner_points={0: [(0, 5, 1.0)]}, dyn_points={0: [(0, 5, 9.0)], 1: "all"})
        t = _run(case, W, H, spawn=2, min_len=1)
        assert len(t.tracks) == 1
        assert (len(t.tracks[0][1]) == 2) == kept
        if kept:   # int(-1.2 + 0.5) = 0: in bounds, and the stored x is negative
            assert t.tracks[0][1][1, 0] == F32(F32(0.0) + F32(dx)) / F32(W) < 0


def test_f32_round_trip_moves_rows():
    W, H = 384, 224
    ia = _ia(W, H)
    y = np.arange(H)
    yq = ((y.astype(F32) / F32(H) * ia).astype(F32) / ia * F32(H)).astype(np.int64)
    assert np.all((yq == y) | (yq == y - 1))
    assert int((yq != y).sum()) == 16 and int(y[yq != y][0]) == 31
    x = np.arange(W)
    assert np.array_equal(((x.astype(F32) / F32(W)).astype(F32) * F32(W)).astype(np.int64), x)
    W2, H2 = 640, 384
    ia2 = _ia(W2, H2)
    y2 = np.arange(H2)
    assert int((((y2.astype(F32) / F32(H2) * ia2).astype(F32) / ia2 * F32(H2)).astype(np.int64) != y2).sum()) == 18
    # row 31 spawns its disk on row 30: with radius 5, (100, 36) is 6 rows away and spawns, (100, 25) is 5 rows away and is
    # refused (from row 31 it would be the other way round)
    assert yq[36] == 36 and yq[25] == 25
    case = _case(2, W, H, corner_points={0: [(100, 31, 3.0), (100, 36, 2.0), (100, 25, 1.0)]},
                 dyn_points={0: [(100, 31, 9.0), (100, 36, 9.0), (100, 25, 9.0)], 1: [(0, 0, 0.0)]})
    t = _run(case, W, H, spawn=5, min_len=1)
    rows = [int(tr[1][0, 1] / ia * H) for tr in t.tracks]
    assert rows == [30, 36]


def test_no_mask_at_frame_zero_and_absent_masks():
    F, W, H = 2, 8, 8
    case = _case(F, W, H, mask=0)
    t = _run(case, W, H, spawn=100, min_len=1, last=1)
    assert len(t.tracks) == 1 and len(t.tracks[0][1]) == 1   # frame 0 spawns (no mask_-00001_000000); mask 0 stops it
    case = _case(3, W, H, mask=0)
    t = _run(case, W, H, spawn=100, min_len=1)
    assert [tr[0] for tr in t.tracks] == [0]                 # frame 1 reads mask_0_1 = 0: no candidate
    case = _case(3, W, H, mask=0, present=1)                 # flows only: continuation needs both, spawning has no mask
    t = _run(case, W, H, spawn=100, min_len=1)
    assert [tr[0] for tr in t.tracks] == [0, 1]


def test_dynamic_distance_tests_ge_and_gt():
    """Continuation accepts dd >= minDynamicDistance, spawning needs dd > minDynamicDistance."""
    F, W, H = 2, 16, 16
    case = _case(F, W, H, flow=(1.0, 0.0), corner_points={0: [(4, 4, 1.0)]}, dyn_points={0: [(4, 4, 9.0)], 1: [(5, 4, 3.0)]})
    t = _run(case, W, H, spawn=1, min_len=1, min_dyn=3)
    assert len(t.tracks) == 1 and len(t.tracks[0][1]) == 2
    case = _case(F, W, H, corner_points={0: [(4, 4, 1.0)]}, dyn_points={0: [(4, 4, 3.0)], 1: "all"})
    assert len(_run(case, W, H, spawn=1, min_len=1, min_dyn=3).tracks) == 0
    assert len(_run(case, W, H, spawn=1, min_len=1, min_dyn=2).tracks) == 1


def test_range_after_zero_and_with_gap():
    F, W, H = 5, 8, 8
    case = _case(F, W, H)
    t = _run(case, W, H, active=[0, 0, 1, 1, 1], first=2, last=4, spawn=100, min_len=1)
    assert [(tr[0], len(tr[1])) for tr in t.tracks] == [(2, 3)]
    t = _run(case, W, H, active=[1, 1, 0, 1, 1], first=0, last=4, spawn=100, min_len=1)
    assert [(tr[0], len(tr[1])) for tr in t.tracks] == [(0, 2), (3, 2)]
    assert t.frame_tracks(2) == []


def test_two_track_table_bytes_and_round_trip(tmp_path):
    t = Table(3, [(1, np.array([[0.25, 0.5], [0.75, 0.125]], np.float32)), None, (0, np.array([[1.0, 2.0]], np.float32))])
    want = (struct.pack("<Q", 3)
            + b"\x01" + struct.pack("<QQ", 1, 2) + struct.pack("<4f", 0.25, 0.5, 0.75, 0.125)
            + b"\x00"
            + b"\x01" + struct.pack("<QQ", 0, 1) + struct.pack("<2f", 1.0, 2.0)
            + struct.pack("<QQ", 0, 3))
    assert serialize(t) == want
    back = deserialize(want)
    assert back == t and serialize(back) == want
    assert back.frame_tracks(0) == [2] and back.frame_tracks(1) == [0] and back.frame_tracks(2) == [0]
    # a computed table too
    F, W, H = 4, 12, 10
    rng = np.random.default_rng(3)
    case = _case(F, W, H, flow=(0.7, -0.4))
    case[0][:] = rng.uniform(0, 1, case[0].shape)
    t = _run(case, W, H, spawn=3, prune=2, min_len=2)
    data = serialize(t)
    assert serialize(deserialize(data)) == data and deserialize(data) == t


def test_import_tracks_csv():
    text = "0, 7, 10, 20\n0,3,40,8\nbad line\n1, 7, 12, 22\n2, 3, 41.5, 9\n"
    t = import_tracks_csv(text, 64)
    assert t.num_frames == 3 and len(t.tracks) == 2
    assert t.tracks[0][0] == 0 and np.array_equal(t.tracks[0][1], np.array([[10, 20], [12, 22]], np.float32) / np.float32(64))
    assert t.tracks[1][0] == 0 and t.tracks[1][1].shape == (2, 2)   # appended as the next frame (TrackBaseSequential)
    with pytest.raises(RuntimeError, match="consecutive"):
        import_tracks_csv("2,1,0,0\n1,1,0,0\n", 64)
