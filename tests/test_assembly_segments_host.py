"""The segment cutter of the assembly's work list (robust_cvd_amd/csrc/cvd_asm_segments.h: cutAsmSegments) without a GPU: a
stand-alone program (tests/asm_segments_main.cpp, which includes that header alone) is compiled with the host compiler and fed
random pair lists -- and the one of tests/test_gpu_assembly_segments.py.  The properties the kernel relies on are checked on its
output directly, and the output is held against the Python statement of the work list (tests/assembly_segments_model.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.assembly_segments_model import UNIT, WAVES, unit_list, work_list

HERE = os.path.dirname(os.path.abspath(__file__))
GPU_TEST_COUNTS = {(0, 1): 641, (0, 2): 850, (0, 3): 65, (0, 4): 641, (0, 5): 641, (0, 6): 63, (1, 0): 800, (1, 2): 800, (2, 0): 641,
                   (2, 1): 768, (3, 0): 512, (3, 4): 257, (4, 0): 64, (4, 3): 257, (5, 0): 129, (5, 2): 800, (6, 0): 63}
SPECIAL = [1, 63, 64, 65, 128, 129, 257, 640]


@pytest.fixture(scope="module")
def cutter(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = tmp_path_factory.mktemp("asm_segments") / "asm_segments"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-o", str(exe), os.path.join(HERE, "asm_segments_main.cpp")],
                   check=True, capture_output=True, timeout=120)

    def run(pairs, counts, frames, cap_units, waves=WAVES, unit=UNIT):
        """-> (units, parts, waveOff, segments as (other, side, first, count, last)) of the C++ cutter on this work list."""
        units, parts = unit_list(pairs, counts, frames, cap_units, unit)
        lines = [f"{waves} {unit} {len(pairs)} {len(units)} {len(parts)}"]
        lines += [f"{a} {b} {n}" for (a, b), n in zip(pairs, counts)]
        lines += [f"{p * 2 + side} {off}" for (p, side, _o, off, _n) in units]
        lines += [f"{u0} {u1}" for (_f, u0, u1) in parts]
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True, timeout=30).stdout
        rows = [ln.split() for ln in out.splitlines()]
        wave_off = [int(t) for t in rows[0][1:]]
        assert rows[0][0] == "W" and all(r[0] == "S" for r in rows[1:])
        return units, parts, wave_off, [tuple(int(t) for t in r[1:]) for r in rows[1:]]
    return run


def check(pairs, counts, frames, cap_units, cutter, waves=WAVES, unit=UNIT):
    units, parts, wave_off, segs = cutter(pairs, counts, frames, cap_units, waves, unit)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    assert len(wave_off) == len(parts) * waves + 1 and wave_off[0] == 0 and wave_off[-1] == len(segs)
    assert all(b >= a for a, b in zip(wave_off, wave_off[1:]))
    covered = {}   # (frame, pair, side) -> list of (first, count) relative to the pair
    empty_waves = 0
    for q, (f, u0, u1) in enumerate(parts):
        per_wave_units = []
        at = u0
        for w in range(waves):
            mine = segs[wave_off[q * waves + w]:wave_off[q * waves + w + 1]]
            empty_waves += 0 if mine else 1
            # the last-of-wave flag: on the wave's last segment and on no other
            assert [s[4] for s in mine] == [0] * (len(mine) - 1) + [1] * (1 if mine else 0)
            n_units = 0
            for (other, side, first, count, _last) in mine:
                assert count > 0
                # the segment continues the part's run exactly where the wave stands: its units are `at`, `at + 1`, ...
                p, uside, uo, uoff, _n = units[at]
                assert (uside, uo) == (side, other) and offsets[p] + uoff == first
                # no segment crosses an entry: it lies inside the constraints of pair p
                assert offsets[p] <= first and first + count <= offsets[p + 1]
                left = count
                while left > 0:
                    assert units[at][:2] == (p, side) and at < u1
                    left -= units[at][4]
                    at += 1
                    n_units += 1
                assert left == 0
                covered.setdefault((f, p, side), []).append((first - offsets[p], count))
            # consecutive segments of a wave are different entries or not contiguous (segments are maximal)
            for s0, s1 in zip(mine, mine[1:]):
                assert not (s0[0] == s1[0] and s0[1] == s1[1] and s0[2] + s0[3] == s1[2])
            per_wave_units.append(n_units)
        assert at == u1
        # each part's waves hold unit counts within one of each other, the larger ones first
        assert max(per_wave_units) - min(per_wave_units) <= 1 and per_wave_units == sorted(per_wave_units, reverse=True)
    # every constraint of every (pair, side) entry lies in exactly one segment
    for p, ((a, b), n) in enumerate(zip(pairs, counts)):
        for f, side in ((a, 0), (b, 1)):
            runs = sorted(covered.pop((f, p, side), []))
            if n == 0 or a == b:
                assert not runs
                continue
            assert runs[0][0] == 0 and sum(c for _, c in runs) == n
            assert all(r0[0] + r0[1] == r1[0] for r0, r1 in zip(runs, runs[1:]))
    assert not covered
    # ... and the list is the model's
    _, model = work_list(pairs, counts, frames, cap_units, waves, unit)
    flat = [(o, side, int(offsets[p]) + first, n) for per_wave in model for sg in per_wave for (p, side, o, first, n) in sg]
    assert flat == [s[:4] for s in segs]
    return empty_waves, [s[3] for s in segs]


def test_the_gpu_tests_problem(cutter):
    pairs = sorted(GPU_TEST_COUNTS)
    empty, lengths = check(pairs, [GPU_TEST_COUNTS[p] for p in pairs], 8, 40, cutter)
    assert empty > 0 and set(SPECIAL) <= set(lengths)


@pytest.mark.parametrize("seed", range(12))
def test_random_pair_lists(cutter, seed):
    rng = np.random.default_rng(seed)
    frames = int(rng.integers(2, 12))
    all_pairs = [(a, b) for a in range(frames) for b in range(frames) if a != b]
    keep = rng.random(len(all_pairs)) < rng.uniform(0.2, 0.9)
    pairs = [p for p, k in zip(all_pairs, keep) if k] or all_pairs[:1]
    counts = [int(rng.choice(SPECIAL)) if rng.random() < 0.5 else int(rng.integers(0, 1500)) for _ in pairs]
    cap = int(rng.choice([8, 9, 16, 24, 40, 137]))
    empty, lengths = check(pairs, counts, frames, cap, cutter)
    assert lengths or not any(counts)
    # another wave count and unit size cut the same way
    check(pairs, counts, frames, cap, cutter, waves=4, unit=64)


def test_empty_waves_and_empty_frames(cutter):
    # three units in all: five of a part's eight waves have no segment; frame 2 has no constraints at all
    empty, lengths = check([(0, 1), (1, 0)], [129, 1], 3, 8, cutter)
    assert lengths == [128, 1, 1, 128, 1, 1] and empty == 8 + 5 + 5
