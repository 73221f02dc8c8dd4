"""Code-generation guard for the epipolar RANSAC kernels (robust_cvd_amd/csrc/cvd_epipolar.h; no GPU needed, hipcc
cross-compiles gfx950): the hypothesis kernel's 8 x 9 elimination (pivots and swaps by selects, every index static) and the
select kernel's Jacobi (a row per lane) stay in registers: no kernel uses scratch memory."""
import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_epipolar.h"
void launch_all(hipStream_t s) {{
  cvd::EpiArgs A{{}};
  hipLaunchKernelGGL(cvd::k_epi_normalise, dim3(1), dim3(256), 0, s, A);
  hipLaunchKernelGGL(cvd::k_epi_hypotheses, dim3(1), dim3(64), 0, s, A);
  hipLaunchKernelGGL(cvd::k_epi_score, dim3(1), dim3(256), 0, s, A);
  hipLaunchKernelGGL(cvd::k_epi_select, dim3(1), dim3(256), 0, s, A);
}}
'''


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_epipolar"))


@pytest.mark.parametrize("name", ["k_epi_normalise", "k_epi_hypotheses", "k_epi_score", "k_epi_select"])
def test_epipolar_kernels_use_no_scratch(asm, name):
    fields, body, _meta = kernel_info(asm, name)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert "scratch_" not in body
