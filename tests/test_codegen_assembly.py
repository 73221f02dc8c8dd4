"""Code-generation guard of the frame-major assembly kernel (no GPU needed: hipcc cross-compiles gfx950).

The benchmarked instantiation of k_assemble_fast -- bilinear grid (KD = 4), list mode, the other frame's parameters staged in LDS,
the default variant fixed at compile time (SPEC = 1) -- must keep everything in registers: no scratch segment and no spilled
VGPR (the standing rule for the fast kernels, tests/test_codegen.py::test_fast_kernels_use_no_scratch).  Its runtime-variant
predecessor carried 128 B of scratch and 29 spilled VGPRs at the 256-register budget of its 8-wave workgroups.

cvd_assembly.h brings two small inline kernels into the unit (k_shared_focal_fixup, k_extract_diag), whose metadata entries come
first in the file: the figures are read from the ONE entry that names this instantiation."""
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info, kernel_names

ARGS = ("Layout, Table, const double*, const FrameConst*, const double*, const float*, const unsigned char*, "
        "const unsigned char*, AsmWork, double*, double*, double*, double*, double*, DenseRecords")
SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_device.h"
#include "{CSRC}/cvd_kernels.h"
#include "{CSRC}/cvd_assembly.h"
namespace cvd {{
template __global__ void k_assemble_fast<4, false, true, false, 1>({ARGS});
}}
'''
KERNEL = "15k_assemble_fastILi4ELb0ELb1ELb0ELi1E"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_assembly"), extra_flags=("-munsafe-fp-atomics",))


def own_metadata(asm, name):
    """{key: int} of the metadata entry (amdhsa.kernels list) of the one kernel whose mangled name contains `name`: every entry
    opens with `- .agpr_count:`, so a kernel's own entry is the piece between two such openings that holds its `.name:`."""
    listing = asm[asm.index("amdhsa.kernels:"):]
    entries = [e for e in re.split(r"^\s*- \.agpr_count:", listing, flags=re.M)[1:]
               if re.search(r"^\s*\.name:\s+\S*" + re.escape(name), e, re.M)]
    assert len(entries) == 1, (name, len(entries))
    entry = entries[0]
    assert len(re.findall(r"^\s*\.name:", entry, re.M)) == 1   # one kernel's entry, not a span over several
    return {k: int(v) for k, v in re.findall(r"^\s*\.(\w+):\s+(\d+)\s*$", entry, re.M)}


def test_metadata_is_read_from_the_assembly_kernels_own_entry(asm):
    """The unit holds other kernels, with a few registers each: the entry picked is the instantiation's."""
    assert len([n for n in kernel_names(asm) if KERNEL in n]) == 1
    # (35 f64 accumulators alone are 70 VGPRs; the helper kernels of the unit have fewer than 32)
    assert own_metadata(asm, KERNEL)["vgpr_count"] >= 70


def test_specialised_assembly_keeps_everything_in_registers(asm):
    fields, _body, _meta = kernel_info(asm, KERNEL)
    meta = own_metadata(asm, KERNEL)
    print("vgpr_count", meta["vgpr_count"], "private_segment_fixed_size", meta["private_segment_fixed_size"],
          "vgpr_spill_count", meta["vgpr_spill_count"], "sgpr_spill_count", meta["sgpr_spill_count"])
    assert meta["private_segment_fixed_size"] == 0 and fields["private_segment_fixed_size"] == 0
    assert meta["vgpr_spill_count"] == 0
    # 8 waves per workgroup, one workgroup per CU (the packed block fills the LDS): two waves per SIMD
    assert meta["vgpr_count"] <= 256 and fields["next_free_vgpr"] <= 256
