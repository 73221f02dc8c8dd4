"""Code-generation guard for the ResNeXt backbone kernels (robust_cvd_amd/csrc/cvd_resnext.h; no GPU needed, hipcc
cross-compiles gfx950): every instantiation the host launches keeps its accumulators and staged loads in registers -- no scratch
memory and no dynamic stack --, stays within a 64 KiB LDS allocation (the grouped convolution uses none), and its register count
leaves the waves per SIMD that DESIGN.md §3.20 states for it.  Checked by the kernel descriptors' fields only."""
import os
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

# (channels per group, stride) of launchRxGroupConv and (filter size, stride, float4 weight loads) of launchRxConv in cvd_frontend.hip
GROUPED = [(cg, s) for cg in (8, 16, 32, 64) for s in (1, 2)]
DENSE = [(7, 2, False), (1, 1, True), (1, 1, False), (1, 2, True), (1, 2, False)]
CHUNK_K = {1: 32, 7: 98}


def grouped_name(instance):
    return "10k_rx_gconvILi%dELi%dEE" % instance


def dense_name(instance):
    ks, stride, vec = instance
    return f"9k_rx_convILi{ks}ELi{stride}ELb{int(vec)}EE"


FOLD = "9k_rx_fold"
POOL = "12k_rx_maxpool"

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_resnext.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_rx_gconv<{cg}, {s}>(RxConvArgs);\n" for cg, s in GROUPED) \
    + "".join(f"template __global__ void k_rx_conv<{ks}, {s}, {str(vec).lower()}>(RxConvArgs);\n" for ks, s, vec in DENSE) + '''
// (the fold and the pool are not templates: taking their address emits them)
__device__ void* const kKeep[] = {reinterpret_cast<void*>(&k_rx_fold), reinterpret_cast<void*>(&k_rx_maxpool)};
}
'''

ALL = [grouped_name(i) for i in GROUPED] + [dense_name(i) for i in DENSE] + [FOLD, POOL]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_resnext"))


@pytest.mark.parametrize("kernel", ALL)
def test_resnext_kernels_use_no_scratch(asm, kernel):
    fields, _body, _meta = kernel_info(asm, kernel)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields
    assert fields["group_segment_fixed_size"] <= 64 * 1024, fields


@pytest.mark.parametrize("instance", GROUPED)
def test_grouped_conv_needs_no_lds_and_keeps_seven_waves(asm, instance):
    """weights enter as wave-uniform operands; two channels' taps, their offsets and two sets of eight accumulators live in
    registers: seven waves a SIMD, 512 // 7 // 8 * 8 = 72"""
    fields, _body, _meta = kernel_info(asm, grouped_name(instance))
    print(f"k_rx_gconv<{instance[0]}, {instance[1]}>: {fields['next_free_vgpr']} VGPR, {fields.get('next_free_sgpr')} SGPR")
    assert fields["group_segment_fixed_size"] == 0, fields
    assert fields["next_free_vgpr"] <= 512 // 7 // 8 * 8, fields


@pytest.mark.parametrize("instance", DENSE)
def test_dense_conv_chunk_fits_the_lds(asm, instance):
    fields, _body, _meta = kernel_info(asm, dense_name(instance))
    ck = CHUNK_K[instance[0]]
    # ck x 64 shifted pixels and the tile's 64 rows of ck weights at an odd stride
    assert (ck * 64 + 64 * ck) * 4 <= fields["group_segment_fixed_size"] <= 64 * 1024, fields


# DESIGN.md §3.20's waves per SIMD (512 registers a SIMD lane, allocated in blocks of 8): the 1 x 1 kernels keep four, as
# k_midas_conv<1> in §3.19; the stem, which holds 25 staged taps and 25 weights per lane behind unrolled address arithmetic, one, as
# k_enc_conv<7> in §3.18.
WAVES = {(7, 2, False): 1, (1, 1, True): 4, (1, 1, False): 4, (1, 2, True): 4, (1, 2, False): 4}


@pytest.mark.parametrize("instance", DENSE)
def test_dense_conv_kernels_keep_their_waves_per_simd(asm, instance):
    fields, _body, _meta = kernel_info(asm, dense_name(instance))
    print(f"k_rx_conv{instance}: {fields['next_free_vgpr']} VGPR, {fields['group_segment_fixed_size']} bytes of LDS")
    assert fields["next_free_vgpr"] <= 512 // WAVES[instance] // 8 * 8, fields


def test_the_elementwise_kernels_keep_a_small_footprint(asm):
    """no LDS, full occupancy (8 waves a SIMD)"""
    for name in (FOLD, POOL):
        fields, _body, _meta = kernel_info(asm, name)
        assert fields["group_segment_fixed_size"] == 0 and fields["next_free_vgpr"] <= 64, (name, fields)


def test_the_front_end_unit_alone_includes_the_header():
    """(tests/test_codegen_units.py's rule for the front-end kernel headers, for this one; and the header stays apart from the other
    front-end kernel headers, whose own guards expect the front end as their only user)"""
    users = [f for f in sorted(os.listdir(CSRC)) if f != "cvd_resnext.h"
             and re.search(r'^#include "cvd_resnext\.h"', open(os.path.join(CSRC, f)).read(), re.M)]
    assert users == ["cvd_frontend.hip"], users
    text = open(os.path.join(CSRC, "cvd_resnext.h")).read()
    assert re.findall(r'^#include "cvd_\w+\.h"', text, re.M) == []
    # `__global__` and `void` on one line, as the other headers (the pattern of tests/test_codegen_units.py stands on it)
    assert len(re.findall(r"\b__global__\b", re.sub(r"//[^\n]*", "", text))) == len(re.findall(r"__global__[^\n;{]*\bvoid\s+\w+\s*\(", text))
