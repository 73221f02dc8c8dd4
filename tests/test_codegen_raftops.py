"""Code-generation guard for the RAFT operators (robust_cvd_amd/csrc/cvd_raftops.h; no GPU needed, hipcc cross-compiles gfx950):
every instantiation the library launches -- the pyramid, the lookup at radius 1..4, the upsampling -- keeps its block, footprint
weights and logits in registers: no scratch memory and no dynamic stack; the lookup's footprints fit a 64 KiB LDS allocation.
Checked by the kernel descriptors' fields only."""
import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

RADII = (1, 2, 3, 4)
KERNELS = ["14k_corr_pyramidE", "17k_convex_upsampleE"] + [f"13k_corr_lookupILi{r}EE" for r in RADII]

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_raftops.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_corr_lookup<{r}>(CorrLookupArgs);\n" for r in RADII) + "}\n"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_raftops"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_raft_kernels_use_no_scratch(asm, kernel):
    fields, _body, _meta = kernel_info(asm, kernel)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields


@pytest.mark.parametrize("radius", RADII)
def test_lookup_footprints_fit_the_lds(asm, radius):
    fields, _body, _meta = kernel_info(asm, f"13k_corr_lookupILi{radius}EE")
    cells = (2 * radius + 2) ** 2
    # 64 queries x an odd stride of floats, plus the 64 anchors
    assert 64 * cells * 4 <= fields["group_segment_fixed_size"] <= 64 * 1024, fields


def test_the_front_end_unit_alone_includes_the_header():
    """(tests/test_codegen_units.py's rule for the front-end kernel headers, for this one: a unit that includes it would emit its
    two non-template kernels)"""
    import os
    import re
    users = [f for f in sorted(os.listdir(CSRC)) if f != "cvd_raftops.h"
             and re.search(r'^#include "cvd_raftops\.h"', open(os.path.join(CSRC, f)).read(), re.M)]
    assert users == ["cvd_frontend.hip"], users


def test_streaming_kernels_use_no_lds(asm):
    for kernel in KERNELS[:2]:
        fields, _body, _meta = kernel_info(asm, kernel)
        assert fields["group_segment_fixed_size"] == 0, (kernel, fields)
