"""Code-generation guard for the backward kernels of the MiDaS decoder's layers (robust_cvd_amd/csrc/cvd_midas_grad.h, DESIGN.md
§3.21; no GPU needed, hipcc cross-compiles gfx950): every instantiation the host launches keeps its accumulator sets, its column
tables and its staged chunk's loads in registers -- no scratch memory and no dynamic stack --, its LDS fits a 64 KiB allocation, and
its register count leaves the waves per SIMD that DESIGN.md §3.21 states for it.  Checked by the kernel descriptors' fields only."""
import os
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

WGRAD = {1: "13k_midas_wgradILi1EE", 3: "13k_midas_wgradILi3EE"}
FLIP = ("13k_midas_wflipILi1EE", "13k_midas_wflipILi3EE")
UPSAMPLE = ("23k_midas_upsample2x_gradILb0EE", "23k_midas_upsample2x_gradILb1EE")
PLAIN = ("18k_midas_dgrad_fold", "18k_midas_wgrad_fold", "17k_midas_bias_grad")
HEAD = ("17k_midas_head_gradE", "21k_midas_head_grad_sum")         # launched by the head's backward

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_midas_grad.h"
namespace cvd {{
template __global__ void k_midas_wgrad<1>(MidasWgradArgs);
template __global__ void k_midas_wgrad<3>(MidasWgradArgs);
template __global__ void k_midas_wflip<1>(MidasFlipArgs);
template __global__ void k_midas_wflip<3>(MidasFlipArgs);
template __global__ void k_midas_upsample2x_grad<false>(MidasUpsampleGradArgs);
template __global__ void k_midas_upsample2x_grad<true>(MidasUpsampleGradArgs);
// (not templates: taking their addresses emits them)
__device__ void* const kKeep[] = {{reinterpret_cast<void*>(&k_midas_dgrad_fold), reinterpret_cast<void*>(&k_midas_wgrad_fold),
                                  reinterpret_cast<void*>(&k_midas_bias_grad), reinterpret_cast<void*>(&k_midas_head_grad),
                                  reinterpret_cast<void*>(&k_midas_head_grad_sum)}};
}}
'''


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_midas_grad"))


@pytest.mark.parametrize("kernel", list(WGRAD.values()) + list(FLIP) + list(UPSAMPLE) + list(PLAIN) + list(HEAD))
def test_grad_kernels_use_no_scratch(asm, kernel):
    fields, _body, _meta = kernel_info(asm, kernel)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields
    assert fields["group_segment_fixed_size"] <= 64 * 1024, fields


@pytest.mark.parametrize("ks", [1, 3])
def test_wgrad_keeps_its_lds_and_its_waves_per_simd(asm, ks):
    """LDS: 64 rows x 33 and 32 pixels x 65 floats.  DESIGN.md §3.21's waves per SIMD (512 registers a SIMD lane, allocated in blocks
    of 8): four for the 1 x 1 filter, three for the 3 x 3 one (its columns carry a channel, a tap offset and a tap index each), as
    the forward's float4 kernels in §3.19."""
    fields, body, _meta = kernel_info(asm, WGRAD[ks])
    print(f"k_midas_wgrad<{ks}>: {fields['next_free_vgpr']} VGPR, {fields['group_segment_fixed_size']} bytes of LDS")
    assert fields["group_segment_fixed_size"] == (64 * 33 + 32 * 65) * 4, fields
    assert fields["next_free_vgpr"] <= 512 // {1: 4, 3: 3}[ks] // 8 * 8, fields
    assert body.count("v_mfma_f32_32x32x2_f32") >= 8          # the chunk's MFMA loop, unrolled by 8


def test_the_elementwise_kernels_keep_a_small_footprint(asm):
    """no LDS (the bias reduction: its 256 f64 sums), full occupancy (8 waves a SIMD)"""
    for name in FLIP + UPSAMPLE + PLAIN:
        fields, _body, _meta = kernel_info(asm, name)
        lds = 256 * 8 if name == PLAIN[2] else 0
        print(f"{name}: {fields['next_free_vgpr']} VGPR")
        assert fields["group_segment_fixed_size"] == lds and fields["next_free_vgpr"] <= 64, (name, fields)


def test_the_head_kernels_keep_a_small_footprint(asm):
    """The pointwise kernel holds one pixel per thread and reduces 33 f64 values through the wave: the four waves' sums in the LDS
    (4 x 33 doubles), full occupancy; the sum kernel no LDS."""
    fields, _body, _meta = kernel_info(asm, HEAD[0])
    print(f"k_midas_head_grad: {fields['next_free_vgpr']} VGPR, {fields['group_segment_fixed_size']} bytes of LDS")
    assert fields["group_segment_fixed_size"] == 4 * 33 * 8 and fields["next_free_vgpr"] <= 64, fields
    fields, _body, _meta = kernel_info(asm, HEAD[1])
    print(f"k_midas_head_grad_sum: {fields['next_free_vgpr']} VGPR")
    assert fields["group_segment_fixed_size"] == 0 and fields["next_free_vgpr"] <= 64, fields


def test_the_front_end_unit_alone_includes_the_header():
    users = [f for f in sorted(os.listdir(CSRC)) if f != "cvd_midas_grad.h"
             and re.search(r'^#include "cvd_midas_grad\.h"', open(os.path.join(CSRC, f)).read(), re.M)]
    assert users == ["cvd_frontend.hip"], users
    text = open(os.path.join(CSRC, "cvd_midas_grad.h")).read()
    assert not re.search(r'^#include "cvd_', text, re.M)           # it stands apart from cvd_midas.h and every other kernel header
    # `__global__` and `void` on one line, as the other headers (the pattern of tests/test_codegen_units.py stands on it)
    assert len(re.findall(r"\b__global__\b", re.sub(r"//[^\n]*", "", text))) == len(re.findall(r"__global__[^\n;{]*\bvoid\s+\w+\s*\(", text))
