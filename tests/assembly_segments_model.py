"""Python statement of the work list of k_assemble_fast's segment walk (robust_cvd_amd/csrc/cvd_setup.hip: units and parts;
cvd_asm_segments.h: segments), for tests that must know which segments a problem produces.  Independent of the C++ text: the CPU
test (tests/test_assembly_segments_host.py) holds the C++ cutter against it, the GPU test compares its segment count with the
kernel launch's."""

UNIT = 128   # kAsmUnit
WAVES = 8    # kAsmThreads / 64


def frame_entries(pairs, counts, frames):
    """Per frame: its (pair, side) entries in table order as (pair index, side, other frame, constraints); empty pairs have none."""
    out = [[] for _ in range(frames)]
    for p, ((a, b), n) in enumerate(zip(pairs, counts)):
        if n <= 0 or a == b:
            continue
        out[a].append((p, 0, b, n))
        out[b].append((p, 1, a, n))
    return out


def unit_list(pairs, counts, frames, cap_units, unit=UNIT):
    """-> (units, parts): every frame's units in frame order, a unit = (pair, side, other, first constraint within the pair,
    constraints); parts = [(frame, u0, u1)] in launch order (longest first, stable), at most cap_units units each."""
    units, parts = [], []
    for f, entries in enumerate(frame_entries(pairs, counts, frames)):
        first = len(units)
        units += [(p, side, o, off, min(unit, n - off)) for (p, side, o, n) in entries for off in range(0, n, unit)]
        nu = len(units) - first
        np_ = max(1, -(-nu // cap_units))
        per = -(-nu // np_)
        for q in range(np_):
            parts.append((f, first + min(nu, q * per), first + min(nu, (q + 1) * per)))
    parts.sort(key=lambda part: -(part[2] - part[1]))   # (stable, as std::stable_sort)
    return units, parts


def work_list(pairs, counts, frames, cap_units, waves=WAVES, unit=UNIT):
    """-> (parts, segments): parts = [(frame, [units])] in launch order; segments = per part, per wave, a list of
    (pair, side, other, first constraint within the pair, count)."""
    all_units, ranges = unit_list(pairs, counts, frames, cap_units, unit)
    parts = [(f, all_units[u0:u1]) for f, u0, u1 in ranges]
    segments = []
    for _, units in parts:
        base, rem = divmod(len(units), waves)
        at, per_wave = 0, []
        for w in range(waves):
            mine = units[at:at + base + (1 if w < rem else 0)]
            at += len(mine)
            segs = []
            for (p, side, o, off, n) in mine:
                if segs and segs[-1][0] == p and segs[-1][1] == side and segs[-1][3] + segs[-1][4] == off:
                    segs[-1] = (p, side, o, segs[-1][3], segs[-1][4] + n)
                else:
                    segs.append((p, side, o, off, n))
            per_wave.append(segs)
        segments.append(per_wave)
    return parts, segments


def properties(pairs, counts, frames, cap_units):
    """What the segment walk meets on this problem: the set of segment lengths, the kinds of transition inside a wave's run, parts per
    frame, waves without a segment."""
    parts, segments = work_list(pairs, counts, frames, cap_units)
    lengths, other_changes, side_flips, mid_entry, idle = set(), 0, 0, 0, 0
    for per_wave in segments:
        for segs in per_wave:
            idle += 0 if segs else 1
            for k, (p, side, o, first, n) in enumerate(segs):
                lengths.add(n)
                mid_entry += 1 if first > 0 else 0
                if k > 0:
                    other_changes += 1 if segs[k - 1][2] != o else 0
                    side_flips += 1 if segs[k - 1][2] == o and segs[k - 1][1] != side else 0
    per_frame = [sum(1 for f, _ in parts if f == g) for g in range(frames)]
    return {"lengths": lengths, "other_changes": other_changes, "side_flips": side_flips, "mid_entry_starts": mid_entry,
            "idle_waves": idle, "parts_per_frame": per_frame, "parts_with_fewer_units_than_waves":
            sum(1 for _, u in parts if 0 < len(u) < WAVES), "segments": sum(len(s) for pw in segments for s in pw),
            "parts": len(parts)}
