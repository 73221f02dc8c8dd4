"""Code-generation guards of the pair product's fixed cost per work item (no GPU needed: hipcc cross-compiles gfx950).

A workgroup of k_matvec_pairs_fast lives ~15 us, of which the constraint loop is ~9: the rest is latency outside the loop.  The
prologue requests every global load it needs into registers before its first wait, the item is described by one 64-byte
record read with one scalar load, and nothing behind the loop's, the reduction's or the write-out's barriers loads from
global memory any more.  Read off the compiled kernels:
  * the register budget of the specialised list instantiations (four waves per SIMD: <= 128 VGPRs, nothing spilled),
  * no global / flat / scalar load after the last LDS atomic of the constraint loop: the epilogue only stores,
  * fewer full vector-memory waits (`s_waitcnt vmcnt(0)`) in front of the first barrier than the parent of this change had.

The full waits that are left in front of the first barrier all belong to the fused coarse gather (CoarseView::Wb != nullptr, off
by default: coarseFrameCorrection's two loops and its mode byte, once per frame), which the default path jumps over with a uniform
branch; the default path itself waits with partial counts only, once every load has been requested.  Where the compiler lays that
block out behind the barrier (the 128-thread instantiation) one full wait is left.
"""
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

SIG = ("(Layout, Table, Items, const double*, const FrameConst*, const double*, const double*, const double*, const double*, int, "
       "double*, CoarseView)")
# (KD, NT, SPEC) -> full vector waits in front of the first barrier.  The parent of this change had 8 in every one of the four
# instantiations that have a barrier (its loads of V.cF, of V.tl -- one wait per trip of a loop --, of the tap table and of
# x / z / p_old / mask each sat in a divergent block in front of the LDS store they fed), 9 loads behind the last LDS atomic
# (frame constants for the pose-row fix-up, the item's ranges and row slots) and the same register counts within two VGPRs.
FULL_WAITS = {(4, 256, 1): 6, (4, 128, 1): 1, (1, 256, 1): 6, (4, 256, 2): 6, (4, 64, 1): None}
PARENT_FULL_WAITS = 8

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_device.h"
#include "{CSRC}/cvd_kernels.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_matvec_pairs_fast<{kd}, {nt}, {spec}>{SIG};\n" for kd, nt, spec in FULL_WAITS) + "}\n"

LOAD = re.compile(r"^\s*(global_load|flat_load|s_load|s_buffer_load|buffer_load|scratch_load)", re.M)


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_prologue"), extra_flags=("-munsafe-fp-atomics",))


def _kernel(asm, inst):
    kd, nt, spec = inst
    return kernel_info(asm, f"19k_matvec_pairs_fastILi{kd}ELi{nt}ELi{spec}ELb0")


@pytest.mark.parametrize("inst", list(FULL_WAITS), ids=lambda i: "kd%d-nt%d-spec%d" % i)
def test_register_budget(asm, inst):
    """Four waves per SIMD; the prologue's loads (EPT = 4 elements of eight vectors per thread at 64 threads) fit beside nothing
    else, because none of the loop's state is live yet."""
    fields, _body, meta = _kernel(asm, inst)
    assert fields["next_free_vgpr"] <= 128, fields
    assert fields["private_segment_fixed_size"] == 0, fields
    spilled = re.search(r"\.vgpr_spill_count:\s*(\d+)", meta)
    assert spilled is not None and int(spilled.group(1)) == 0, meta
    sgpr = re.search(r"\.sgpr_spill_count:\s*(\d+)", meta)
    assert sgpr is not None and int(sgpr.group(1)) <= 31, meta   # (the parent's count: SGPR spills are lane writes, not memory)


@pytest.mark.parametrize("inst", list(FULL_WAITS), ids=lambda i: "kd%d-nt%d-spec%d" % i)
def test_epilogue_only_stores(asm, inst):
    """Behind the last LDS atomic of the constraint loop (KD = 1 keeps its depth-block sums in registers and has none: behind
    the first of the reduction's three barriers) the kernel loads nothing from memory: t, fy and J_l of the pose-row fix-up come
    from the prologue's LDS copy, the output rows from the item's record."""
    _fields, body, _meta = _kernel(asm, inst)
    last = body.rfind("ds_add_f64")
    if last < 0:
        assert inst[0] == 1, "only the Global level has no LDS atomics"
        barriers = [m.start() for m in re.finditer(r"s_barrier", body)]
        assert len(barriers) >= 3
        last = barriers[-3]
    tail = body[last:]
    assert LOAD.findall(tail) == [], LOAD.findall(tail)
    assert "global_store" in tail


@pytest.mark.parametrize("inst", [i for i, n in FULL_WAITS.items() if n is not None], ids=lambda i: "kd%d-nt%d-spec%d" % i)
def test_prologue_full_waits(asm, inst):
    """(One-wave workgroups -- the deterministic build's <4, 64, 1> -- compile without any s_barrier: the region is not
    defined for them; their budget and epilogue are checked above.)"""
    _fields, body, _meta = _kernel(asm, inst)
    prologue = body[:body.index("s_barrier")]
    full = len(re.findall(r"s_waitcnt[^\n]*vmcnt\(0\)", prologue))
    print(f"{inst}: {full} full vector waits in front of the first barrier (parent: {PARENT_FULL_WAITS})")
    assert full < PARENT_FULL_WAITS
    assert full <= FULL_WAITS[inst]
