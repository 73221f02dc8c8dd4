"""Code-generation guard for the update block's convolution kernel (robust_cvd_amd/csrc/cvd_raftconv.h; no GPU
needed, hipcc cross-compiles gfx950): every instantiation the host launches keeps its two accumulator sets and its staged chunk's
loads in registers -- no scratch memory and no dynamic stack --, its staged chunk (shifted pixels and weights) fits a 64 KiB LDS
allocation, and its register count leaves the waves per SIMD that DESIGN.md §3.17 states for it.  Checked by the kernel
descriptors' fields only."""
import os
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

# (filter size, float4 weight loads) of launchRaftConv in cvd_frontend.hip, and the chunk's k = channels x taps
INSTANCES = {(1, True): 32, (1, False): 32, (3, True): 72, (3, False): 72, (7, False): 98}
KERNELS = {f"11k_raft_convILi{ks}ELb{int(vec)}EE": ck for (ks, vec), ck in INSTANCES.items()}

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_raftconv.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_raft_conv<{ks}, {'true' if vec else 'false'}>(ConvArgs);\n" for ks, vec in INSTANCES) + "}\n"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_raftconv"))


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_conv_kernels_use_no_scratch(asm, kernel):
    fields, _body, _meta = kernel_info(asm, kernel)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_conv_chunk_fits_the_lds(asm, kernel):
    fields, _body, _meta = kernel_info(asm, kernel)
    ck = KERNELS[kernel]
    # ck x 64 shifted pixels and 64 rows of ck weights at an odd stride
    assert (ck * 64 + 64 * ck) * 4 <= fields["group_segment_fixed_size"] <= 64 * 1024, fields


# DESIGN.md §3.17's waves per SIMD: the two float4 kernels that carry the block's 3 x 3 and 1 x 1 layers keep three and four, the
# scalar-weight fallback of the 3 x 3 filter two, the 7 x 7 filter (49 taps in flight per lane, 0.8 % of the block's FLOP) one.
WAVES = {(1, True): 4, (1, False): 4, (3, True): 3, (3, False): 2, (7, False): 1}


@pytest.mark.parametrize("instance", list(INSTANCES))
def test_conv_kernels_keep_their_waves_per_simd(asm, instance):
    """(512 registers a SIMD lane, allocated in blocks of 8)"""
    ks, vec = instance
    fields, _body, _meta = kernel_info(asm, f"11k_raft_convILi{ks}ELb{int(vec)}EE")
    assert fields["next_free_vgpr"] <= 512 // WAVES[instance] // 8 * 8, fields


def test_the_front_end_unit_alone_includes_the_header():
    """(tests/test_codegen_units.py's rule for the front-end kernel headers, for this one)"""
    users = [f for f in sorted(os.listdir(CSRC)) if f != "cvd_raftconv.h"
             and re.search(r'^#include "cvd_raftconv\.h"', open(os.path.join(CSRC, f)).read(), re.M)]
    assert users == ["cvd_frontend.hip"], users
