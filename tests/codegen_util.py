"""Harness of the code-generation guards (tests/test_codegen*.py; no GPU needed, hipcc cross-compiles gfx950): compile a source
text to device assembly and pick one kernel's descriptor, body and metadata out of it."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robust_cvd_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def device_asm(source_text, tmp_dir, extra_flags=()):
    """gfx950 assembly text of `source_text` (`hipcc -O3 -S --cuda-device-only`); skips the calling test when hipcc is absent."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    src, out = tmp_dir / "k.hip", tmp_dir / "k.s"
    src.write_text(source_text)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", *extra_flags, "-S", "--cuda-device-only", "-o", str(out),
                    str(src)], check=True, capture_output=True, timeout=600)
    return out.read_text()


def kernel_names(asm):
    """Mangled names of every kernel in the assembly."""
    return re.findall(r"\.amdhsa_kernel (\S+)\n", asm)


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
