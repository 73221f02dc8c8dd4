"""Code-generation guard for the backbone's training kernels (robust_cvd_amd/csrc/cvd_resnext_grad.h; no GPU
needed, hipcc cross-compiles gfx950): every instantiation the host launches keeps its accumulators in registers -- no scratch memory
and no dynamic stack -- and stays within a 64 KiB LDS allocation.  Checked by the kernel descriptors' fields only; the register
counts are printed."""
import os
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

# (channels per group, stride) of launchRxgGroupDgradK and (filter size, stride) of launchRxgWgradK in cvd_frontend.hip
DGRAD = [(cg, s) for cg in (8, 16, 32, 64) for s in (1, 2)]
WGRAD = [(3, 1), (3, 2), (7, 2)]
PLAIN = ["k_rxg_norm_stats", "k_rxg_norm_finish", "k_rxg_norm_apply", "k_rxg_norm_grad_sums", "k_rxg_norm_grad_finish",
         "k_rxg_norm_grad_apply", "k_rxg_wgrad_fold", "k_rxg_gather2", "k_rxg_scatter2", "k_rxg_maxpool_grad"]
REDUCTIONS = ("k_rxg_norm_stats", "k_rxg_norm_grad_sums")


def dgrad_name(instance):
    return "17k_rxg_gconv_dgradILi%dELi%dEE" % instance


def wgrad_name(instance):
    return "11k_rxg_wgradILi%dELi%dEE" % instance


def plain_name(name):
    return f"{len(name)}{name}"


SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_resnext_grad.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_rxg_gconv_dgrad<{cg}, {s}>(RxgConvArgs);\n" for cg, s in DGRAD) \
    + "".join(f"template __global__ void k_rxg_wgrad<{ks}, {s}>(RxgConvArgs);\n" for ks, s in WGRAD) + '''
// (the others are not templates: taking their address emits them)
__device__ void* const kKeep[] = {''' + ", ".join(f"reinterpret_cast<void*>(&{n})" for n in PLAIN) + '''};
}
'''

ALL = [dgrad_name(i) for i in DGRAD] + [wgrad_name(i) for i in WGRAD] + [plain_name(n) for n in PLAIN]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_resnext_grad"))


@pytest.mark.parametrize("kernel", ALL)
def test_kernels_use_no_scratch(asm, kernel):
    fields, _body, _meta = kernel_info(asm, kernel)
    print(f"{kernel}: {fields['next_free_vgpr']} VGPR, {fields.get('next_free_sgpr')} SGPR, {fields['group_segment_fixed_size']} bytes of LDS")
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields
    assert fields["group_segment_fixed_size"] <= 64 * 1024, fields


@pytest.mark.parametrize("instance", DGRAD)
def test_grouped_input_gradient_needs_no_lds(asm, instance):
    """weights enter as wave-uniform operands, as in the forward"""
    fields, _body, _meta = kernel_info(asm, dgrad_name(instance))
    assert fields["group_segment_fixed_size"] == 0, fields


def test_only_the_reductions_use_the_lds(asm):
    """256 doubles of the fixed tree"""
    for name in PLAIN:
        fields, _body, _meta = kernel_info(asm, plain_name(name))
        assert fields["group_segment_fixed_size"] == (256 * 8 if name in REDUCTIONS else 0), (name, fields)


def test_the_front_end_unit_alone_includes_the_header():
    users = [f for f in sorted(os.listdir(CSRC)) if f != "cvd_resnext_grad.h"
             and re.search(r'^#include "cvd_resnext_grad\.h"', open(os.path.join(CSRC, f)).read(), re.M)]
    assert users == ["cvd_frontend.hip"], users
    text = open(os.path.join(CSRC, "cvd_resnext_grad.h")).read()
    assert re.findall(r'^#include "cvd_\w+\.h"', text, re.M) == []
    # the kernel map that names this header's kernels is the front-end unit's opening comment (cvd_kernels.h's own map stays as it
    # is: its text is hashed into the committed counter measurements of the pair product, tests/test_profiles.py)
    unit = open(os.path.join(CSRC, "cvd_frontend.hip")).read()
    assert "cvd_resnext_grad.h: k_rxg_norm_stats" in unit[:unit.index("#include")]
    # `__global__` and `void` on one line, as the other headers (the pattern of tests/test_codegen_units.py stands on it)
    assert len(re.findall(r"\b__global__\b", re.sub(r"//[^\n]*", "", text))) == len(re.findall(r"__global__[^\n;{]*\bvoid\s+\w+\s*\(", text))
