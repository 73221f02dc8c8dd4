"""Code-generation guard for the parameter regulariser and the optimizer step (robust_cvd_amd/csrc/cvd_paramstep.h; no GPU needed,
hipcc cross-compiles gfx950): every instantiation the library launches moves 16 bytes per lane on the aligned path (dwordx4
global loads and stores: four f32 or two f64), keeps its elements in registers (no scratch memory, no dynamic stack) and
accumulates nothing atomically (the loss repeats bit for bit)."""
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

TYPES = ("float", "double")

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_paramstep.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_param_l1<{t}>(ParamTable, double*);\n"
              f"template __global__ void k_param_l1_grad<{t}, false>(ParamTable, double, const {t}*);\n"
              f"template __global__ void k_param_l1_grad<{t}, true>(ParamTable, double, const {t}*);\n"
              f"template __global__ void k_param_step<{t}>(ParamTable);\n" for t in TYPES) \
    + "const void* param_l1_finish() { return reinterpret_cast<const void*>(&k_param_l1_finish); }\n}\n"

L1 = [f"10k_param_l1I{t[0]}E" for t in TYPES]
GRAD = [f"15k_param_l1_gradI{t[0]}Lb{a}EE" for t in TYPES for a in (0, 1)]
STEP = [f"12k_param_stepI{t[0]}E" for t in TYPES]
FINISH = ["17k_param_l1_finish"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_paramstep"), extra_flags=["-munsafe-fp-atomics"])


@pytest.mark.parametrize("name", L1 + GRAD + STEP + FINISH)
def test_kernels_use_no_scratch_and_no_atomics(asm, name):
    fields, body, _meta = kernel_info(asm, name)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields
    assert not re.search(r"atomic", body), re.findall(r"\S*atomic\S*", body)[:4]


@pytest.mark.parametrize("name", L1 + GRAD + STEP)
def test_aligned_path_loads_16_bytes_per_lane(asm, name):
    """l1: p and p0; its gradient: p, p0 (and the table it adds to); the step: p, g, m, v."""
    _fields, body, _meta = kernel_info(asm, name)
    loads = len(re.findall(r"\bglobal_load_dwordx4\b", body))
    want = {"10": 2, "15": 3 if "Lb1" in name else 2, "12": 4}[name[:2]]
    assert loads >= want, (name, loads, want)


@pytest.mark.parametrize("name", GRAD + STEP)
def test_aligned_path_stores_16_bytes_per_lane(asm, name):
    """the gradient: one table; the step: p, m, v."""
    _fields, body, _meta = kernel_info(asm, name)
    stores = len(re.findall(r"\bglobal_store_dwordx4\b", body))
    assert stores >= (3 if name.startswith("12") else 1), (name, stores)
