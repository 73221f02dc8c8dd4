"""Code-generation guard for the bilateral filter (robust_cvd_amd/csrc/cvd_bilateral.h; no GPU needed, hipcc cross-compiles
gfx950): the mean kernels and the thread-per-pixel median, whose (depth, weight) samples and sorting network must stay in
VGPRs (every array index a compile-time constant), use no scratch memory."""
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
#include "{CSRC}/cvd_bilateral.h"
namespace cvd {{
template __global__ void k_bilateral_mean<false, false>(BilateralArgs);
template __global__ void k_bilateral_mean<true, true>(BilateralArgs);
template __global__ void k_bilateral_median_small<16, false>(BilateralArgs);
template __global__ void k_bilateral_median_small<64, true>(BilateralArgs);
template __global__ void k_bilateral_median_wave<true>(BilateralArgs, int);
}}
'''


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("codegen_bilateral")
    src, out = d / "k.hip", d / "k.s"
    src.write_text(SOURCE)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    str(src)], check=True, capture_output=True, timeout=600)
    return out.read_text()


def kernel_info(asm, name):
    """(.amdhsa descriptor fields, body text) of the one kernel whose mangled name contains `name`."""
    m = [b for b in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S) if name in b[0]]
    assert len(m) == 1, (name, [b[0] for b in m])
    mangled, desc = m[0]
    fields = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", desc)}
    body = asm[asm.index(f"\n{mangled}:"):]
    body = body[:body.index("s_endpgm")]
    return fields, body


@pytest.mark.parametrize("name", ["16k_bilateral_meanILb0ELb0E", "16k_bilateral_meanILb1ELb1E",
                                  "24k_bilateral_median_smallILi16ELb0E", "24k_bilateral_median_smallILi64ELb1E",
                                  "23k_bilateral_median_waveILb1E"])
def test_bilateral_kernels_use_no_scratch(asm, name):
    fields, body = kernel_info(asm, name)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert "scratch_" not in body
