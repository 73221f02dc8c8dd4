"""Code-generation guard for the bilateral filter (robust_cvd_amd/csrc/cvd_bilateral.h; no GPU needed, hipcc cross-compiles
gfx950): the mean kernels and the thread-per-pixel median, whose (depth, weight) samples and sorting network must stay in
VGPRs (every array index a compile-time constant), use no scratch memory."""
import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_bilateral.h"
namespace cvd {{
template __global__ void k_bilateral_mean<false, false>(BilateralArgs);
template __global__ void k_bilateral_mean<true, true>(BilateralArgs);
template __global__ void k_bilateral_median_small<16, false>(BilateralArgs);
template __global__ void k_bilateral_median_small<64, true>(BilateralArgs);
template __global__ void k_bilateral_median_wave<true>(BilateralArgs, int);
}}
'''


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_bilateral"))


@pytest.mark.parametrize("name", ["16k_bilateral_meanILb0ELb0E", "16k_bilateral_meanILb1ELb1E",
                                  "24k_bilateral_median_smallILi16ELb0E", "24k_bilateral_median_smallILi64ELb1E",
                                  "23k_bilateral_median_waveILb1E"])
def test_bilateral_kernels_use_no_scratch(asm, name):
    fields, body, _meta = kernel_info(asm, name)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert "scratch_" not in body
