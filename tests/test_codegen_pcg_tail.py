"""Code-generation guards of the fused PCG tail (no GPU needed: hipcc cross-compiles gfx950).

k_pcg_tail<KD> runs 768-thread workgroups, two per CU (amdgpu_waves_per_eu(6)): at most 80 VGPRs, and nothing of what its first wave
holds while it releases the grid barrier, or of what a temporal level's wave copies to LDS in front of it, may be bought with spilled
registers or scratch.

Parent of the change that shortened the tail's chain (same recipe): k_pcg_tail<1> / <4> 79 VGPRs, 0 spilled, 0 B scratch, 19 SGPR
spills; k_cg_update 79 VGPRs, 0 spilled, 0 B scratch; k_matvec_finish<4> 63 VGPRs, 0 spilled, 0 B scratch.  The two kernels that share
bodies with the tail must use no more scratch than that.
"""
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_device.h"
#include "{CSRC}/cvd_kernels.h"
#include "{CSRC}/cvd_pcg.h"
namespace cvd {{
template __global__ void k_pcg_tail<1>(Layout, const double*, const double*, const double*, const float*, const unsigned char*,
                                       const unsigned char*, const int*, const int*, const double*, const double*, double*, double*,
                                       int, double*, double*, int, RegCache, CoarseView, double*, const double*, TailUpdate);
template __global__ void k_pcg_tail<4>(Layout, const double*, const double*, const double*, const float*, const unsigned char*,
                                       const unsigned char*, const int*, const int*, const double*, const double*, double*, double*,
                                       int, double*, double*, int, RegCache, CoarseView, double*, const double*, TailUpdate);
template __global__ void k_matvec_finish<4>(Layout, const double*, const double*, const double*, const float*, const unsigned char*,
                                            const unsigned char*, const int*, const int*, const double*, const double*, const double*,
                                            double*, double*, unsigned int*, int, double*, double*, int, int, RegCache, CoarseView,
                                            double*, CoarseColumns, const double*, double*, int, int, const TlStep*);
}}
'''
PARENT_SCRATCH = {"11k_cg_update": 0, "15k_matvec_finishILi4E": 0}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_pcg_tail"), extra_flags=("-munsafe-fp-atomics",))


@pytest.mark.parametrize("kd", [1, 4])
def test_fused_tail_register_budget(asm, kd):
    fields, _body, meta = kernel_info(asm, f"10k_pcg_tailILi{kd}E")
    spilled = re.search(r"\.vgpr_spill_count:\s*(\d+)", meta)
    sgpr = re.search(r"\.sgpr_spill_count:\s*(\d+)", meta)
    print(f"k_pcg_tail<{kd}>: next_free_vgpr {fields['next_free_vgpr']}, scratch {fields['private_segment_fixed_size']} B, "
          f"{sgpr.group(1) if sgpr else '?'} SGPR spills (lane writes, not memory)")
    assert fields["next_free_vgpr"] <= 80, fields
    assert spilled is not None and int(spilled.group(1)) == 0, meta
    assert fields["private_segment_fixed_size"] == 0, fields


@pytest.mark.parametrize("name", list(PARENT_SCRATCH))
def test_kernels_sharing_the_tails_bodies_use_no_more_scratch(asm, name):
    fields, _body, _meta = kernel_info(asm, name)
    assert fields["private_segment_fixed_size"] <= PARENT_SCRATCH[name], fields
