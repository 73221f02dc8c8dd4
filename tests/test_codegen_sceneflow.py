"""Code-generation guard for the scene-flow loss (robust_cvd_amd/csrc/cvd_sceneflow.h; no GPU needed, hipcc cross-compiles
gfx950): every instantiation the library launches -- forward and backward in f32 and f64 with one or four pixels per thread, the
deterministic backward walk, the two finishing kernels -- keeps its samples in registers: no scratch memory and no dynamic
stack, read from the kernel descriptors."""
import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

PASSES = [(k, t, p) for k in ("forward", "backward") for t in ("float", "double") for p in (1, 4)]
DET = ["float", "double"]

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_sceneflow.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_sf_{k}<{t}, {p}>(SfArgs<{t}>);\n" for k, t, p in PASSES) \
    + "".join(f"template __global__ void k_sf_backward_det<{t}>(SfArgs<{t}>);\n" for t in DET) \
    + "".join(f"template __global__ void k_sf_finish_total<{t}>(SfFinishArgs, const {t}*);\n" for t in DET) \
    + "const void* sf_finish_pairs() { return reinterpret_cast<const void*>(&k_sf_finish_pairs); }\n}\n"

NAMES = [f"{len('k_sf_' + k)}k_sf_{k}I{t[0]}Li{p}E" for k, t, p in PASSES] \
    + [f"17k_sf_backward_detI{t[0]}E" for t in DET] + [f"17k_sf_finish_totalI{t[0]}E" for t in DET] + ["17k_sf_finish_pairs"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_sceneflow"), extra_flags=["-munsafe-fp-atomics"])


@pytest.mark.parametrize("name", NAMES)
def test_scene_flow_kernels_use_no_scratch(asm, name):
    fields, _body, _meta = kernel_info(asm, name)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields
