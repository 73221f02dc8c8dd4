"""Code-generation guard for the flow consistency masks (robust_cvd_amd/csrc/cvd_flowmask.h; no GPU needed, hipcc cross-compiles
gfx950): every instantiation the library launches -- 1..4 colour channels, one or four pixels per thread -- keeps its flows,
colours and errors in registers: no scratch memory, no dynamic stack, no LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robust_cvd_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VARIANTS = [(c, p) for c in (1, 2, 3, 4) for p in (1, 4)]

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_flowmask.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_flow_masks<{c}, {p}>(FlowMaskArgs);\n" for c, p in VARIANTS) + "}\n"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("codegen_flowmask")
    src, out = d / "k.hip", d / "k.s"
    src.write_text(SOURCE)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                    str(src)], check=True, capture_output=True, timeout=600)
    return out.read_text()


def kernel_info(asm, name):
    """(.amdhsa descriptor fields, body text, metadata text) of the one kernel whose mangled name contains `name`."""
    m = [b for b in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S) if name in b[0]]
    assert len(m) == 1, (name, [b[0] for b in m])
    mangled, desc = m[0]
    fields = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)", desc)}
    body = asm[asm.index(f"\n{mangled}:"):]
    body = body[:body.index("s_endpgm")]
    meta = re.search(r"- \.agpr_count:.*?\.name:\s+" + re.escape(mangled) + r"\n.*?\.wavefront_size", asm, re.S)
    return fields, body, meta.group(0) if meta else ""


@pytest.mark.parametrize("channels,pixels", VARIANTS)
def test_flow_mask_kernels_use_no_scratch(asm, channels, pixels):
    fields, body, _meta = kernel_info(asm, f"12k_flow_masksILi{channels}ELi{pixels}E")
    assert fields["private_segment_fixed_size"] == 0, fields
    assert fields.get("uses_dynamic_stack", 0) == 0, fields
    assert fields["group_segment_fixed_size"] == 0, fields
    assert "scratch_" not in body
    # the own flow of the four-pixel map is read with 16-byte loads, its mask written with one dword store
    if pixels == 4:
        assert "global_load_dwordx4" in body and "global_store_dword " in body
