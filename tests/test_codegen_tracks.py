"""Code-generation guard for the feature-track kernels (robust_cvd_amd/csrc/cvd_tracks.h; no GPU needed, hipcc
cross-compiles gfx950): the walk keeps its per-lane state in registers and its masks and survivor lists in LDS, so no
kernel uses scratch memory."""
import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

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
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_tracks"))


@pytest.mark.parametrize("name", KERNELS)
def test_track_kernels_use_no_scratch(asm, name):
    fields, body, _meta = kernel_info(asm, name)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert "scratch_" not in body
