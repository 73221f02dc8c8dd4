"""Seeded inputs of the parameter-regulariser and optimizer-step tests (robust_cvd_amd/csrc/cvd_paramstep.h), the
configurations the fixture tests/golden/reference_py/optimizer_golden.npz records, and the elements it records them at.

One table of twelve tensors in flat arrays: 0, 1, 3, 4, 5, 63, 64 and 65 elements (nothing, less than a 16-byte group, a group
and its neighbours, a wave and its neighbours), then PARAM_CHUNK - 1, PARAM_CHUNK, PARAM_CHUNK + 1 and 2 PARAM_CHUNK + 7 (a
chunk's end, two and three chunks, tails of 1 and 7 elements; five chunks' worth of elements, more workgroups than one).  Every
tensor starts at a multiple of four elements of the flat arrays except MISALIGNED, the one of PARAM_CHUNK + 1 elements, which
starts one element later: contiguous, but not 16-byte aligned in either precision.  Every real input is a float32-representable
number held in float64: parameters of order 1, initial values a percent away and EQUAL to the parameter on every third element
(ties), eight gradients with signs and magnitudes log-uniform in [1e-4, 1].

The update rules are element-wise, so the fixture records the reference at SAMPLE elements only -- the first and last eight of
every tensor, eight either side of every chunk boundary and a stride through the rest -- and the whole-array f32 spread as
scalars; the GPU tests check every element in f64 against the restatement (tests/optimizer_reference.py).
"""
import hashlib

import numpy as np

from robust_cvd_amd import api

SEED = 9301
STEPS = 8
RECORDED_STEPS = (1, 5, 6, 8)           # p after these steps (the RAdam regime switches between 5 and 6); m, v after the last
MISALIGNED = 10
LAMBDA = 0.37
GRAD_OUT = 1.5
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)
# name -> (rule family, weight_decay, degenerated_to_sgd)
CONFIGS = {
    "adam-wd0": ("adam", 0.0, None), "adam-wd0.01": ("adam", 0.01, None),
    "radam-wd0-sgd": ("radam", 0.0, True), "radam-wd0.01-sgd": ("radam", 0.01, True),
    "radam-wd0-moments": ("radam", 0.0, False), "radam-wd0.01-moments": ("radam", 0.01, False),
}


def sizes():
    c = api.PARAM_CHUNK
    return [0, 1, 3, 4, 5, 63, 64, 65, c - 1, c, c + 1, 2 * c + 7]


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


_CACHE = {}


def make_case():
    """dict: counts, offsets [T] int64, total (flat length), p, p0 [total] and g [STEPS, total] float64.  Elements of the flat
    arrays between the tensors hold 7 (p, p0) and 0.5 (g): nothing may read or change them.  Cached: callers must not modify it."""
    if "case" in _CACHE:
        return _CACHE["case"]
    counts = np.array(sizes(), np.int64)
    offsets, at = [], 0
    for t, n in enumerate(counts):
        at = (at + 3) // 4 * 4 + (t == MISALIGNED)
        offsets.append(at)
        at += int(n)
    offsets = np.array(offsets, np.int64)
    total = (at + 3) // 4 * 4
    rng = np.random.default_rng(SEED)
    p = _f32(rng.normal(0.0, 1.0, total))
    p0 = _f32(p * (1.0 + 0.01 * rng.normal(0.0, 1.0, total)))
    p0[::3] = p[::3]
    g = _f32(rng.choice([-1.0, 1.0], (STEPS, total)) * 10.0 ** rng.uniform(-4.0, 0.0, (STEPS, total)))
    used = np.zeros(total, bool)
    for o, n in zip(offsets, counts):
        used[o:o + n] = True
    p[~used], p0[~used], g[:, ~used] = 7.0, 7.0, 0.5
    case = dict(counts=counts, offsets=offsets, total=total, p=p, p0=p0, g=g, used=used)
    _CACHE["case"] = case
    return case


def digest(case):
    h = hashlib.sha256()
    for k in ("counts", "offsets", "p", "p0", "g"):
        h.update(np.ascontiguousarray(case[k]).tobytes())
    return h.hexdigest()


def tensors(case, flat):
    """The tensors of a flat array (views)."""
    return [flat[o:o + n] for o, n in zip(case["offsets"], case["counts"])]


def sample_indices(case):
    """Flat indices of the elements the fixture records, ascending."""
    c = api.PARAM_CHUNK
    pick = set()
    for o, n in zip(case["offsets"].tolist(), case["counts"].tolist()):
        local = set(range(min(8, n))) | set(range(max(n - 8, 0), n)) | set(range(0, n, 257))
        for b in range(c, n, c):
            local |= set(range(b - 8, min(b + 8, n)))
        pick |= {o + i for i in local}
    return np.array(sorted(pick), np.int64)
