"""Code-generation guard for the encoder kernels (robust_cvd_amd/csrc/cvd_raftenc.h; no GPU needed, hipcc
cross-compiles gfx950): every instantiation the host launches keeps its two accumulator sets and its staged chunk's loads in
registers -- no scratch memory and no dynamic stack --, its staged chunk (shifted pixels and weights) fits a 64 KiB LDS allocation,
and its register count leaves the waves per SIMD that DESIGN.md §3.18 states for it.  Checked by the kernel descriptors' fields
only."""
import os
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

# (filter size, stride, float4 weight loads) of launchEncConv in cvd_frontend.hip, and the chunk's k = channels x taps
CHUNK_K = {1: 32, 3: 72, 7: 98}
INSTANCES = [(ks, stride, vec) for ks in (1, 3) for stride in (1, 2) for vec in (True, False)] + [(7, 1, False), (7, 2, False)]


def mangled(instance):
    ks, stride, vec = instance
    return f"10k_enc_convILi{ks}ELi{stride}ELb{int(vec)}EE"


NORM_KERNELS = ("16k_instnorm_stats", "16k_instnorm_apply")

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_raftenc.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_enc_conv<{ks}, {stride}, {'true' if vec else 'false'}>(EncConvArgs);\n"
              for ks, stride, vec in INSTANCES) + '''
// (the two norm kernels are not templates: taking their addresses emits them)
__device__ void* const kKeep[] = {reinterpret_cast<void*>(&k_instnorm_stats), reinterpret_cast<void*>(&k_instnorm_apply)};
}
'''


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_raftenc"))


@pytest.mark.parametrize("kernel", [mangled(i) for i in INSTANCES] + list(NORM_KERNELS))
def test_encoder_kernels_use_no_scratch(asm, kernel):
    fields, _body, _meta = kernel_info(asm, kernel)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields
    assert fields["group_segment_fixed_size"] <= 64 * 1024, fields


@pytest.mark.parametrize("instance", INSTANCES)
def test_conv_chunk_fits_the_lds(asm, instance):
    fields, _body, _meta = kernel_info(asm, mangled(instance))
    ck = CHUNK_K[instance[0]]
    # ck x 64 shifted pixels and 64 rows of ck weights at an odd stride
    assert (ck * 64 + 64 * ck) * 4 <= fields["group_segment_fixed_size"] <= 64 * 1024, fields


def test_the_norm_kernels_keep_a_small_footprint(asm):
    """one f64 per thread of LDS for the statistics' tree, none for the elementwise pass; both at full occupancy (8 waves a SIMD)"""
    stats, _body, _meta = kernel_info(asm, NORM_KERNELS[0])
    apply_, _body, _meta = kernel_info(asm, NORM_KERNELS[1])
    assert stats["group_segment_fixed_size"] == 256 * 8 and apply_["group_segment_fixed_size"] == 0
    assert stats["next_free_vgpr"] <= 64 and apply_["next_free_vgpr"] <= 64


# DESIGN.md §3.18's waves per SIMD (512 registers a SIMD lane, allocated in blocks of 8), as for k_raft_conv in §3.17: the float4
# kernels that carry the encoder's 3 x 3 and 1 x 1 layers keep three and four, the scalar-weight fallback of the 3 x 3 filter two,
# the 7 x 7 filter (conv1: 49 taps in flight per lane) one.
WAVES = {(1, True): 4, (1, False): 4, (3, True): 3, (3, False): 2, (7, False): 1}


@pytest.mark.parametrize("instance", INSTANCES)
def test_conv_kernels_keep_their_waves_per_simd(asm, instance):
    ks, stride, vec = instance
    fields, _body, _meta = kernel_info(asm, mangled(instance))
    print(f"k_enc_conv<{ks}, {stride}, {vec}>: {fields['next_free_vgpr']} VGPR, {fields['group_segment_fixed_size']} bytes of LDS")
    assert fields["next_free_vgpr"] <= 512 // WAVES[(ks, vec)] // 8 * 8, fields


def test_the_front_end_unit_alone_includes_the_header():
    """(tests/test_codegen_units.py's rule for the front-end kernel headers, for this one; and the header stays apart from
    cvd_raftconv.h, whose own guard expects the front end as its only user)"""
    users = [f for f in sorted(os.listdir(CSRC)) if f != "cvd_raftenc.h"
             and re.search(r'^#include "cvd_raftenc\.h"', open(os.path.join(CSRC, f)).read(), re.M)]
    assert users == ["cvd_frontend.hip"], users
    assert "#include \"cvd_raftconv.h\"" not in open(os.path.join(CSRC, "cvd_raftenc.h")).read()
