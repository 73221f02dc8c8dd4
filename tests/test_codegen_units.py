"""Code-generation guard for the translation units (no GPU needed, hipcc cross-compiles gfx950): the front-end kernel headers
are included by cvd_frontend.hip alone.  A unit that includes one of them parses it and emits device code for every
non-template kernel in it; cvd_comm.hip, the exchange layer, launches k_local_sum only and stands for the other eight units."""
import os
import re

import pytest

from robust_cvd_amd import build
from tests.codegen_util import CSRC, device_asm, kernel_names

FRONTEND_HEADERS = ["cvd_dense.h", "cvd_sampling.h", "cvd_imageops.h", "cvd_filter.h", "cvd_bilateral.h", "cvd_epipolar.h",
                    "cvd_tracks.h", "cvd_flowmask.h", "cvd_consistency.h", "cvd_sceneflow.h", "cvd_spatial.h"]
# (cvd_loss_common.h, which the three loss headers include, defines device functions only: no kernel to look for)


def header_kernels(header):
    """Names of the `__global__` functions a header defines."""
    with open(os.path.join(CSRC, header)) as f:
        return re.findall(r"__global__\s+(?:__launch_bounds__\(\w+\)\s+)?void\s+(\w+)\s*\(", f.read())


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(f'#include "{CSRC}/cvd_comm.hip"\n', tmp_path_factory.mktemp("codegen_units"), extra_flags=build.FLAGS)


def test_exchange_layer_holds_no_front_end_kernel(asm):
    names = kernel_names(asm)
    assert any("11k_local_sum" in n for n in names), names   # the unit's own kernel: the list is the unit's
    for header in FRONTEND_HEADERS:
        kernels = header_kernels(header)
        assert kernels, header
        for k in kernels:
            assert not [n for n in names if f"{len(k)}{k}" in n], (header, k)
