"""Workload-shaped item lists for the pair product at test size (plain numpy, no GPU).

The parity tests of the matrix-free product (k_matvec_pairs_fast / k_matvec_pairs, robust_cvd_amd/csrc/cvd_kernels.h) run on videos
of 4 to 8 frames: the host cuts their pairs down to 128-constraint chunks (compileTable, cvd_setup.hip) and launches a few dozen
work items, always at 256 threads (launchMatvec, cvd_matvec.hip).  The cases here reach, at 64x40 pixels, what only full-size
solves reached before:
  * at least 3 x 256 undirected pairs, so the 768-constraint chunk of the sampled lists stays uncut on a 256-CU device,
  * 850 / 1090 work items: inside or outside the 128-thread window of every (KD, SPEC) variant of the fast kernel,
  * a handful of LONG pairs at the chunk edges (one item of exactly 768 constraints, 769 -> two items, both directions split,
    a direction that is absent, a direction much longer than the other), the rest thinned to 3 - 24 constraints per direction.

`expected_items` and `expected_threads` restate the host's two rules so that a test can tell which kernel instantiation a case is
meant to run, and notice when a rule changes under it.
"""
import functools

import numpy as np

from robust_cvd_amd import synth

WIDTH, HEIGHT = 64, 40
MAX_OFFSET = 8          # pairs (i, i + o) and (i + o, i) for o = 1 .. 8
LONG_SPACING = 1.7      # ~1000 constraints per directed pair at 64x40
SHORT_SPACING = 7.0     # ~60 candidates per directed pair, thinned to 3 - 24
LIST_CHUNK = 768        # kListChunk (cvd_host.h): constraints per direction and work item, list mode
MIN_CHUNK = 128
MAX_LDS = 160 * 1024    # kMaxLds (cvd_host.h)
FRAME_CONST_BYTES = 49 * 8                 # sizeof(FrameConst) (cvd_device.h)
RED_DOUBLES = 32 + 15 * (4 * 33 + 1)       # red[32] + kRedVals x kRedStride (cvd_kernels.h)

CASES = {"items850": {"frames": 110, "seed": 850}, "items1090": {"frames": 140, "seed": 1090}}

# Long pairs: name -> (offset of the pair, constraints a -> b, constraints b -> a) with a < b; None = the whole dense slice
# (~1000), "absent" = the directed pair is not in the list at all.  Each sits on an undirected pair of its own.
EDGES = {
    "one_item_768_and_1": (1, 768, 1),              # one item, three trips of 256 threads (six of 128) in one direction
    "two_items_769": (2, 769, 12),                  # 769 -> items of 385 and 384; the short direction is split 6 + 6
    "both_directions_split": (1, None, None),       # ~1000 / ~1000 -> two items of ~500 in both directions
    "reverse_absent": (3, None, "absent"),          # ~1000 forward, no b -> a pair: items with an empty direction
    "long_backward_5_forward": (4, 5, None),        # ~1000 backward and 5 forward: items of 3 + ~500 and 2 + ~500
}


def edge_frames(name, num_frames):
    """(a, b), a < b, of the long pair `name`: spread over the video, away from its ends."""
    k = list(EDGES).index(name)
    a = (k + 1) * num_frames // (len(EDGES) + 2)
    return a, a + EDGES[name][0]


def _all_pairs(num_frames):
    pairs = []
    for o in range(1, MAX_OFFSET + 1):
        for i in range(num_frames - o):
            pairs += [(i, i + o), (i + o, i)]
    return sorted(pairs)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """SyntheticVideo of the case: the scene, cameras and depth maps of synth.make_video; its constraint list is assembled from
    a sparse sampling of every pair (thinned) and a dense sampling of the long pairs (cut to their exact lengths)."""
    F, seed = CASES[name]["frames"], CASES[name]["seed"]
    rng = np.random.default_rng(seed + 1)
    long_dirs, absent = {}, set()
    for ename, (_, n_fwd, n_bwd) in EDGES.items():
        a, b = edge_frames(ename, F)
        for (src, dst), n in (((a, b), n_fwd), ((b, a), n_bwd)):
            if n == "absent":
                absent.add((src, dst))
            elif n is None or n > 24:
                long_dirs[(src, dst)] = n
    pairs = [p for p in _all_pairs(F) if p not in absent]
    # (same seed, frame count and size: both calls draw the same scene, cameras and depth maps before any constraint)
    short = synth.make_video(F, WIDTH, HEIGHT, seed=seed, pairs=pairs, spacing=SHORT_SPACING)
    dense = synth.make_video(F, WIDTH, HEIGHT, seed=seed, pairs=sorted(long_dirs), spacing=LONG_SPACING)
    assert np.array_equal(short.depth, dense.depth)
    dense_index = {tuple(p): k for k, p in enumerate(dense.pairs.tolist())}
    exact = {}
    for ename, (_, n_fwd, n_bwd) in EDGES.items():
        a, b = edge_frames(ename, F)
        for key, n in (((a, b), n_fwd), ((b, a), n_bwd)):
            if isinstance(n, int):
                exact[key] = n
    chunks, off = [], [0]
    for k, p in enumerate(short.pairs.tolist()):
        key = tuple(p)
        if key in long_dirs:
            d = dense_index[key]
            loc = dense.loc[dense.offsets[d]:dense.offsets[d + 1]]
        else:
            loc = short.loc[short.offsets[k]:short.offsets[k + 1]]
        if key in exact:
            want = exact[key]
        elif key in long_dirs:
            want = loc.shape[0]
        else:
            # most pairs keep 3 - 24; one in sixteen keeps up to 40 (more than half a wave, less than one)
            want = int(rng.integers(3, 25)) if rng.uniform() > 1.0 / 16 else int(rng.integers(25, 41))
        assert loc.shape[0] >= min(want, 3), (name, key, loc.shape[0], want)
        if key in exact:
            assert loc.shape[0] >= want, (name, key, loc.shape[0], want)
        want = min(want, loc.shape[0])
        keep = np.sort(rng.choice(loc.shape[0], size=want, replace=False))   # (spread over the image, list order kept)
        chunks.append(loc[keep])
        off.append(off[-1] + want)
    short.loc = np.ascontiguousarray(np.concatenate(chunks, axis=0))
    short.offsets = np.asarray(off, dtype=np.int64)
    short.is_static = np.ones(short.loc.shape[0], dtype=np.uint8)
    short.meta = dict(short.meta, case=name, spacing=(SHORT_SPACING, LONG_SPACING))
    return short


def pair_counts(video):
    """{(a, b): constraints} of every directed pair of the list."""
    n = np.diff(video.offsets)
    return {tuple(p): int(c) for p, c in zip(video.pairs.tolist(), n)}


def expected_items(video, num_cu):
    """The work items compileTable (cvd_setup.hip, list mode, all frames in range) makes of the video's pair list on a device
    of num_cu compute units: [(fa, fb, constraints fa -> fb, constraints fb -> fa)], longest first as they are launched."""
    edges = {}
    for (a, b), n in pair_counts(video).items():
        if a == b or n <= 0:
            continue
        e = edges.setdefault((min(a, b), max(a, b)), [0, 0])
        e[0 if a < b else 1] = n
    longest = sum(max(n0, n1) for n0, n1 in edges.values())
    chunk = LIST_CHUNK
    slots = 3 * num_cu
    if longest // LIST_CHUNK + len(edges) < slots:   # the items would not fill the device once: cut finer, down to 128
        want = (longest + slots - 1) // slots
        chunk = min(LIST_CHUNK, max(MIN_CHUNK, (want + 63) // 64 * 64))
    items = []
    for (fa, fb) in sorted(edges):
        n0, n1 = edges[(fa, fb)]
        n_items = max(1, (max(n0, n1) + chunk - 1) // chunk)
        c0, c1 = (n0 + n_items - 1) // n_items, (n1 + n_items - 1) // n_items
        for k in range(n_items):
            m0 = min(n0, (k + 1) * c0) - min(n0, k * c0)
            m1 = min(n1, (k + 1) * c1) - min(n1, k * c1)
            if m0 <= 0 and m1 <= 0:
                continue
            items.append((fa, fb, m0, m1))
    items.sort(key=lambda it: -(it[2] + it[3]))   # (stable, like the host's)
    return items


def expected_threads(kd, spec, block, num_cu, n_items):
    """Threads per workgroup launchMatvec (cvd_matvec.hip) picks for the fast list kernel <kd, NT, spec> with frame blocks of
    `block` unknowns: 256 when the items fit into one round of 256-thread workgroups or need more than one round of 128-thread
    ones, else 128."""
    waves_per_simd = (4 if kd <= 4 else 3) if spec else 2
    lds_fast = 6 * block * 8 + 2 * FRAME_CONST_BYTES + RED_DOUBLES * 8
    slots256 = waves_per_simd * num_cu
    slots128 = min(2 * slots256, (MAX_LDS // lds_fast) * num_cu)
    return 256 if (n_items <= slots256 or n_items > slots128) else 128
