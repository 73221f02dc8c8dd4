"""Code-generation guard for the MiDaS decoder kernels (robust_cvd_amd/csrc/cvd_midas.h; no GPU needed, hipcc
cross-compiles gfx950): every instantiation the host launches keeps its two accumulator sets and its staged chunk's loads in
registers -- no scratch memory and no dynamic stack --, its staged chunk (shifted pixels and weights) fits a 64 KiB LDS allocation,
and its register count leaves the waves per SIMD that DESIGN.md §3.19 states for it.  Checked by the kernel descriptors' fields
only."""
import os
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

# (filter size, float4 weight loads, head) of launchMidasConv and launchMidasHead in cvd_frontend.hip
INSTANCES = [(1, True, False), (1, False, False), (3, True, False), (3, False, False), (3, True, True), (3, False, True)]
CHUNK_K = {1: 32, 3: 72}


def mangled(instance):
    ks, vec, head = instance
    return f"12k_midas_convILi{ks}ELb{int(vec)}ELb{int(head)}EE"


UPSAMPLE = ("18k_midas_upsample2xILb0EE", "18k_midas_upsample2xILb1EE")
FOLD = "12k_midas_fold"

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_midas.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_midas_conv<{ks}, {str(vec).lower()}, {str(head).lower()}>(MidasConvArgs);\n"
              for ks, vec, head in INSTANCES) + '''
template __global__ void k_midas_upsample2x<false>(MidasUpsampleArgs);
template __global__ void k_midas_upsample2x<true>(MidasUpsampleArgs);
// (the fold is not a template: taking its address emits it)
__device__ void* const kKeep[] = {reinterpret_cast<void*>(&k_midas_fold)};
}
'''


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_midas"))


@pytest.mark.parametrize("kernel", [mangled(i) for i in INSTANCES] + list(UPSAMPLE) + [FOLD])
def test_midas_kernels_use_no_scratch(asm, kernel):
    fields, _body, _meta = kernel_info(asm, kernel)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields
    assert fields["group_segment_fixed_size"] <= 64 * 1024, fields


@pytest.mark.parametrize("instance", INSTANCES)
def test_conv_chunk_fits_the_lds(asm, instance):
    fields, _body, _meta = kernel_info(asm, mangled(instance))
    ck = CHUNK_K[instance[0]]
    pixels, channels = (128, 32) if instance[2] else (64, 64)
    # ck x pixels shifted pixels and the tile's rows of ck weights at an odd stride
    assert (ck * pixels + channels * ck) * 4 <= fields["group_segment_fixed_size"] <= 64 * 1024, fields


def test_the_elementwise_kernels_keep_a_small_footprint(asm):
    """no LDS, full occupancy (8 waves a SIMD)"""
    for name in UPSAMPLE + (FOLD,):
        fields, _body, _meta = kernel_info(asm, name)
        assert fields["group_segment_fixed_size"] == 0 and fields["next_free_vgpr"] <= 64, (name, fields)


# DESIGN.md §3.19's waves per SIMD (512 registers a SIMD lane, allocated in blocks of 8): the float4 kernels that carry the decoder
# keep four (1 x 1) and three (3 x 3), the scalar-weight fallback of the 3 x 3 filter two, as k_enc_conv in §3.18; the head, which
# holds four channels' taps per lane for its 128-pixel tile, three with float4 weights and two without.
WAVES = {(1, True, False): 4, (1, False, False): 4, (3, True, False): 3, (3, False, False): 2, (3, True, True): 3, (3, False, True): 2}


@pytest.mark.parametrize("instance", INSTANCES)
def test_conv_kernels_keep_their_waves_per_simd(asm, instance):
    ks, vec, head = instance
    fields, _body, _meta = kernel_info(asm, mangled(instance))
    print(f"k_midas_conv<{ks}, {vec}, {head}>: {fields['next_free_vgpr']} VGPR, {fields['group_segment_fixed_size']} bytes of LDS")
    assert fields["next_free_vgpr"] <= 512 // WAVES[instance] // 8 * 8, fields


def test_the_front_end_unit_alone_includes_the_header():
    """(tests/test_codegen_units.py's rule for the front-end kernel headers, for this one; and the header stays apart from
    cvd_raftenc.h and cvd_raftconv.h, whose own guards expect the front end as their only user)"""
    users = [f for f in sorted(os.listdir(CSRC)) if f != "cvd_midas.h"
             and re.search(r'^#include "cvd_midas\.h"', open(os.path.join(CSRC, f)).read(), re.M)]
    assert users == ["cvd_frontend.hip"], users
    text = open(os.path.join(CSRC, "cvd_midas.h")).read()
    assert "#include \"cvd_raftconv.h\"" not in text and "#include \"cvd_raftenc.h\"" not in text
    # `__global__` and `void` on one line, as the other headers (the pattern of tests/test_codegen_units.py stands on it)
    assert len(re.findall(r"\b__global__\b", re.sub(r"//[^\n]*", "", text))) == len(re.findall(r"__global__[^\n;{]*\bvoid\s+\w+\s*\(", text))
