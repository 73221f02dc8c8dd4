"""Code-generation guard for the SepConvGRU kernels (robust_cvd_amd/csrc/cvd_raftgru.h; no GPU needed, hipcc cross-compiles
gfx950): both launches of a half keep their two accumulator sets in registers -- no scratch memory and no dynamic stack -- and
their staged chunk (shifted pixels and weights) fits a 64 KiB LDS allocation.  Checked by the kernel descriptors' fields only."""
import os
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

KERNELS = ["10k_gru_gemmILb0EE", "10k_gru_gemmILb1EE"]

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_raftgru.h"
namespace cvd {{
template __global__ void k_gru_gemm<false>(GruArgs);
template __global__ void k_gru_gemm<true>(GruArgs);
}}
'''


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_raftgru"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_gru_kernels_use_no_scratch(asm, kernel):
    fields, _body, _meta = kernel_info(asm, kernel)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields


@pytest.mark.parametrize("kernel", KERNELS)
def test_gru_chunk_fits_the_lds(asm, kernel):
    fields, _body, _meta = kernel_info(asm, kernel)
    # 80 x 64 shifted pixels and 64 rows of 80 weights at an odd stride
    assert (80 * 64 + 64 * 80) * 4 <= fields["group_segment_fixed_size"] <= 64 * 1024, fields


@pytest.mark.parametrize("kernel", KERNELS)
def test_gru_kernels_keep_three_waves_per_simd(asm, kernel):
    """(three workgroups of a CU overlap one's staging with the others' MFMA; 512 registers / 3 waves)"""
    fields, _body, _meta = kernel_info(asm, kernel)
    assert fields["next_free_vgpr"] <= 168, fields


def test_the_front_end_unit_alone_includes_the_header():
    """(tests/test_codegen_units.py's rule for the front-end kernel headers, for this one)"""
    users = [f for f in sorted(os.listdir(CSRC)) if f != "cvd_raftgru.h"
             and re.search(r'^#include "cvd_raftgru\.h"', open(os.path.join(CSRC, f)).read(), re.M)]
    assert users == ["cvd_frontend.hip"], users
