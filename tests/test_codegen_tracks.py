"""Code-generation guard for the feature-track kernels (robust_cvd_amd/csrc/cvd_tracks.h; no GPU needed, hipcc
cross-compiles gfx950): the walk keeps its per-lane state in registers and its masks and survivor lists in LDS, so no
kernel uses scratch memory."""
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
#include "{CSRC}/cvd_tracks.h"
void launch_all(hipStream_t s) {{
  cvd::TrackArgs A{{}};
  cvd::TrackBufs B{{}};
  hipLaunchKernelGGL(cvd::k_track_candidates, dim3(1), dim3(256), 0, s, A, 0, nullptr, nullptr);
  hipLaunchKernelGGL(cvd::k_track_walk, dim3(1), dim3(cvd::kTrackThreads), 0, s, A, 0, 1, nullptr, nullptr, B, nullptr);
  hipLaunchKernelGGL(cvd::k_track_lengths, dim3(1), dim3(256), 0, s, 0, nullptr, nullptr);
  hipLaunchKernelGGL(cvd::k_track_keep, dim3(1), dim3(256), 0, s, 0, 0, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(cvd::k_track_scatter, dim3(1), dim3(256), 0, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr, nullptr);
}}
'''

KERNELS = ["k_track_candidates", "k_track_walk", "k_track_lengths", "k_track_keep", "k_track_scatter"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("codegen_tracks")
    src, out = d / "k.hip", d / "k.s"
    src.write_text(SOURCE)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    str(src)], check=True, capture_output=True, timeout=600)
    return out.read_text()


@pytest.mark.parametrize("name", KERNELS)
def test_track_kernels_use_no_scratch(asm, name):
    m = [b for b in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S) if name in b[0]]
    assert len(m) == 1, (name, [b[0] for b in m])
    mangled, desc = m[0]
    fields = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", desc)}
    assert fields["private_segment_fixed_size"] == 0, fields
    body = asm[asm.index(f"\n{mangled}:"):]
    assert "scratch_" not in body[:body.index("s_endpgm")]
