"""Code-generation guard for the epipolar RANSAC kernels (robust_cvd_amd/csrc/cvd_epipolar.h; no GPU needed, hipcc
cross-compiles gfx950): the hypothesis kernel's 8 x 9 elimination (pivots and swaps by selects, every index static) and the
select kernel's Jacobi (a row per lane) stay in registers: no kernel uses scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robust_cvd_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_epipolar.h"
void launch_all(hipStream_t s) {{
  cvd::EpiArgs A{{}};
  hipLaunchKernelGGL(cvd::k_epi_normalise, dim3(1), dim3(256), 0, s, A);
  hipLaunchKernelGGL(cvd::k_epi_hypotheses, dim3(1), dim3(64), 0, s, A);
  hipLaunchKernelGGL(cvd::k_epi_score, dim3(1), dim3(256), 0, s, A);
  hipLaunchKernelGGL(cvd::k_epi_select, dim3(1), dim3(256), 0, s, A);
}}
'''


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("codegen_epipolar")
    src, out = d / "k.hip", d / "k.s"
    src.write_text(SOURCE)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    str(src)], check=True, capture_output=True, timeout=600)
    return out.read_text()


@pytest.mark.parametrize("name", ["k_epi_normalise", "k_epi_hypotheses", "k_epi_score", "k_epi_select"])
def test_epipolar_kernels_use_no_scratch(asm, name):
    m = [b for b in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S) if name in b[0]]
    assert len(m) == 1, (name, [b[0] for b in m])
    mangled, desc = m[0]
    fields = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", desc)}
    assert fields["private_segment_fixed_size"] == 0, fields
    body = asm[asm.index(f"\n{mangled}:"):]
    assert "scratch_" not in body[:body.index("s_endpgm")]
