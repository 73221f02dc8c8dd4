"""Code-generation guard for the spatial losses (robust_cvd_amd/csrc/cvd_spatial.h; no GPU needed, hipcc cross-compiles gfx950):
every instantiation the library launches -- the pass in f32 and f64 with one or four pixels per thread, with and without the
gradient, and the finishing kernel -- keeps its pixels and their neighbours in registers: no scratch memory and no dynamic stack,
read from the kernel descriptors."""
import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

PASSES = [(t, p, g) for t in ("float", "double") for p in (1, 4) for g in (0, 1)]

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_spatial.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_sp_pass<{t}, {p}, {'true' if g else 'false'}>(SpArgs<{t}>);\n" for t, p, g in PASSES) \
    + "const void* sp_finish() { return reinterpret_cast<const void*>(&k_sp_finish); }\n}\n"

NAMES = [f"9k_sp_passI{t[0]}Li{p}ELb{g}EE" for t, p, g in PASSES] + ["11k_sp_finish"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_spatial"), extra_flags=["-munsafe-fp-atomics"])


@pytest.mark.parametrize("name", NAMES)
def test_spatial_kernels_use_no_scratch(asm, name):
    fields, _body, _meta = kernel_info(asm, name)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields
