"""Code-generation guard for the flow consistency masks (robust_cvd_amd/csrc/cvd_flowmask.h; no GPU needed, hipcc cross-compiles
gfx950): every instantiation the library launches -- 1..4 colour channels, one or four pixels per thread -- keeps its flows,
colours and errors in registers: no scratch memory, no dynamic stack, no LDS."""
import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info
VARIANTS = [(c, p) for c in (1, 2, 3, 4) for p in (1, 4)]

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_flowmask.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_flow_masks<{c}, {p}>(FlowMaskArgs);\n" for c, p in VARIANTS) + "}\n"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_flowmask"))


@pytest.mark.parametrize("channels,pixels", VARIANTS)
def test_flow_mask_kernels_use_no_scratch(asm, channels, pixels):
    fields, body, _meta = kernel_info(asm, f"12k_flow_masksILi{channels}ELi{pixels}E")
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields
    assert fields["group_segment_fixed_size"] == 0, fields
    assert "scratch_" not in body
    # the own flow of the four-pixel map is read with 16-byte loads, its mask written with one dword store
    if pixels == 4:
        assert "global_load_dwordx4" in body and "global_store_dword " in body
