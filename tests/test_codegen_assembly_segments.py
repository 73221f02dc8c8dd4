"""Code-generation guard of the segment walk of the frame-major assembly kernel (no GPU needed: hipcc cross-compiles gfx950; the
recipe of tests/codegen_util.py and tests/test_codegen_assembly.py).

The specialised list-mode instantiations of k_assemble_fast walk segments (cvd_assembly.h: asmWalkSegments): the next segment's
record is held across the trips of the current one and the next trip's table record is in flight, in a kernel that sits at its
256-register budget (8 waves per workgroup, two per SIMD).
  * bilinear (KD = 4), Cauchy and Huber: no scratch, no spilled VGPR, at most 256 VGPRs;
  * bicubic (KD = 16): no more spilled VGPRs and scratch than the unit walk it replaces had (Cauchy 11 VGPRs / 48 B, Huber 4 / 20 B);
  * inside the constraint loop of a segment -- the innermost loop that holds the LDS atomics of the accumulation -- no scalar load
    (the segment records, frame constants and kernel arguments are all read outside it) and no `s_waitcnt vmcnt(0)` but the record
    stream's own: one, in front of the first use of the record requested a trip earlier.  The LDS-DMA staging of the next segment's
    parameters is issued from that loop's last trip and waited for outside it.
The unit walk's loop had 0 scalar loads and 7 `s_waitcnt`; the counts of this build are printed beside those."""
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info
from tests.test_codegen_assembly import ARGS, own_metadata

INSTANCES = {  # (KD, SPEC) -> mangled-name piece; list mode, staged, no fold
    (4, 1): "15k_assemble_fastILi4ELb0ELb1ELb0ELi1E", (4, 2): "15k_assemble_fastILi4ELb0ELb1ELb0ELi2E",
    (16, 1): "15k_assemble_fastILi16ELb0ELb1ELb0ELi1E", (16, 2): "15k_assemble_fastILi16ELb0ELb1ELb0ELi2E",
}
SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_device.h"
#include "{CSRC}/cvd_kernels.h"
#include "{CSRC}/cvd_assembly.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_assemble_fast<{kd}, false, true, false, {spec}>({ARGS});\n" for kd, spec in INSTANCES) + "}\n"
UNIT_WALK_SPILLS = {(16, 1): (11, 48), (16, 2): (4, 20)}   # spilled VGPRs, scratch bytes of the unit walk (DESIGN_LOG)
UNIT_WALK_LOOP = {"scalar_loads": 0, "s_waitcnt": 7}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_assembly_segments"), extra_flags=("-munsafe-fp-atomics",))


def constraint_loop(body):
    """Lines of the innermost loop of a kernel body that contains the accumulation's LDS f64 atomics: the span from a label to the
    LAST backward branch to it, the shortest such span with a constraint's atomics in it."""
    lines = body.split("\n")
    label_at = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"(\.LBB\d+_\d+):", ln)] if m}
    spans = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)|\s+s_branch\s+(\.LBB\d+_\d+)", ln)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in label_at and label_at[tgt] < i:
                spans[tgt] = max(spans.get(tgt, 0), i)
    loops = [lines[label_at[t]:end + 1] for t, end in spans.items()]
    # (42 atomics per constraint at four taps, the regularisers' and the fold's loops have a handful; the bicubic taps' atomics sit
    # in an inner loop of their own, which requests no record)
    with_atomics = [lp for lp in loops if sum(1 for ln in lp if "ds_add_f64" in ln) >= 42
                    and any("global_load_dwordx4" in ln for ln in lp)]
    assert with_atomics, "no loop with the accumulation's LDS f64 atomics found"
    return min(with_atomics, key=len)


@pytest.mark.parametrize("kd,spec", sorted(INSTANCES))
def test_registers_and_scratch(asm, kd, spec):
    name = INSTANCES[(kd, spec)]
    fields, _body, _meta = kernel_info(asm, name)
    meta = own_metadata(asm, name)
    print(f"KD {kd} SPEC {spec}: vgpr_count {meta['vgpr_count']} vgpr_spill_count {meta['vgpr_spill_count']} "
          f"private_segment_fixed_size {meta['private_segment_fixed_size']} sgpr_spill_count {meta['sgpr_spill_count']}")
    assert meta["vgpr_count"] <= 256 and fields["next_free_vgpr"] <= 256
    if kd == 4:
        assert meta["vgpr_spill_count"] == 0
        assert meta["private_segment_fixed_size"] == 0 and fields["private_segment_fixed_size"] == 0
    else:
        spilled, scratch = UNIT_WALK_SPILLS[(kd, spec)]
        assert meta["vgpr_spill_count"] <= spilled
        assert meta["private_segment_fixed_size"] <= scratch and fields["private_segment_fixed_size"] <= scratch


@pytest.mark.parametrize("kd,spec", sorted(INSTANCES))
def test_constraint_loop_has_no_scalar_load_and_one_full_vector_wait(asm, kd, spec):
    _fields, body, _meta = kernel_info(asm, INSTANCES[(kd, spec)])
    loop = constraint_loop(body)
    scalar_loads = [ln.strip() for ln in loop if re.match(r"\s+s_(buffer_)?load_", ln)]
    waits = [(i, ln.strip()) for i, ln in enumerate(loop) if re.match(r"\s+s_waitcnt\b", ln)]
    vm_waits = [(i, w) for i, w in waits if "vmcnt" in w]
    vector_loads = sorted(ln.split()[0] for ln in loop if re.match(r"\s+(global|flat|buffer|scratch)_load", ln))
    atomics = [i for i, ln in enumerate(loop) if "ds_add_f64" in ln]
    dma = [i for i, ln in enumerate(loop) if "global_load_lds_dword" in ln]
    print(f"KD {kd} SPEC {spec}: constraint loop {len(loop)} lines, {len(atomics)} LDS atomics, scalar loads {len(scalar_loads)} "
          f"(unit walk {UNIT_WALK_LOOP['scalar_loads']}), s_waitcnt {len(waits)} (unit walk {UNIT_WALK_LOOP['s_waitcnt']}), "
          f"of them on vmcnt {[w for _, w in vm_waits]} at lines {[i for i, _ in vm_waits]}, vector loads {vector_loads}, "
          f"LDS-DMA at line {dma}, atomics in lines {atomics[0]}..{atomics[-1]}")
    assert not scalar_loads, scalar_loads
    # The only vector loads of the loop are the record stream's two and the look-ahead staging's one (no scratch reload either), so
    # every wait on vmcnt is the record stream's own: the staging has no consumer inside the loop ...
    assert vector_loads == ["global_load_dwordx2", "global_load_dwordx4", "global_load_lds_dword"], vector_loads
    # ... and none of them stands between the staging request and the end of the trip's accumulation: a trip never waits for it
    assert len(dma) == 1 and not [i for i, _ in vm_waits if dma[0] < i < atomics[-1]], vm_waits
    assert len(vm_waits) <= 3, vm_waits   # (the record is two loads: one wait each where the next trip takes them over, one at the top)
