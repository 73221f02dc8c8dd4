"""Code-generation guard for the fine-tuning batch kernels (robust_cvd_amd/csrc/cvd_batch.h; no GPU needed, hipcc cross-compiles
gfx950): every instantiation the library launches keeps its values in registers (no scratch memory, no dynamic stack), and the
aligned batch path moves 16 bytes per lane (dwordx4 global loads and stores: colour 3 + 3, flow 2 + 2, tables 1 + 1)."""
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_batch.h"
namespace cvd {{
template __global__ void k_dataset_batch<true>(DatasetStore, DatasetBatch, const long long*, int, unsigned int*);
template __global__ void k_dataset_batch<false>(DatasetStore, DatasetBatch, const long long*, int, unsigned int*);
template __global__ void k_dataset_scale_map<4>(Layout, int, int, const double*, float*);
template __global__ void k_dataset_scale_map<16>(Layout, int, int, const double*, float*);
template __global__ void k_dataset_warp_map<0>(Layout, int, int, const double*, float*);
template __global__ void k_dataset_warp_map<4>(Layout, int, int, const double*, float*);
template __global__ void k_dataset_warp_map<16>(Layout, int, int, const double*, float*);
const void* scale_scalars() {{ return reinterpret_cast<const void*>(&k_dataset_scale_scalars); }}
}}
'''

BATCH = ["15k_dataset_batchILb1EE", "15k_dataset_batchILb0EE"]
TABLES = ["19k_dataset_scale_mapILi4EE", "19k_dataset_scale_mapILi16EE", "18k_dataset_warp_mapILi0EE", "18k_dataset_warp_mapILi4EE",
          "18k_dataset_warp_mapILi16EE", "23k_dataset_scale_scalars"]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_dataset"), extra_flags=["-munsafe-fp-atomics"])


@pytest.mark.parametrize("name", BATCH + TABLES)
def test_kernels_use_no_scratch(asm, name):
    fields, _body, _meta = kernel_info(asm, name)
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields


def _whole_body(asm, name):
    """the kernel's text up to its size directive (kernel_info stops at the first s_endpgm; this kernel has several exits)"""
    m = re.search(r"\n(\S*" + re.escape(name) + r"\S*):[^\n]*\n(.*?)\n\s*\.size\s+\1,", asm, re.S)
    assert m, name
    return m.group(2)


def test_aligned_path_moves_16_bytes_per_lane(asm):
    body = _whole_body(asm, BATCH[0])
    loads = len(re.findall(r"\bglobal_load_dwordx4\b", body))
    stores = len(re.findall(r"\bglobal_store_dwordx4\b", body))
    assert loads >= 6, loads
    assert stores >= 6, stores
