"""Code-generation guard for the translation units (no GPU needed, hipcc cross-compiles gfx950).  A unit that includes a kernel
header parses it and emits device code for every non-template kernel in it, launched or not.  So: the front-end kernel headers
are included by cvd_frontend.hip alone; cvd_host.h, which every unit includes, brings no non-template kernel at all; and a unit
includes, by name, the headers of the kernels it launches and no others.  cvd_comm.hip, the exchange layer, launches k_local_sum
only; cvd_solve, cvd_api and cvd_temporal are the units whose compile is short enough to check here (the five heavy units were
checked once by hand: DESIGN_LOG.md)."""
import os
import re

import pytest

from robust_cvd_amd import build
from tests.codegen_util import CSRC, device_asm, kernel_names

FRONTEND_HEADERS = ["cvd_dense.h", "cvd_sampling.h", "cvd_imageops.h", "cvd_filter.h", "cvd_bilateral.h", "cvd_epipolar.h",
                    "cvd_tracks.h", "cvd_flowmask.h", "cvd_consistency.h", "cvd_sceneflow.h", "cvd_spatial.h"]
# (cvd_loss_common.h, which the three loss headers include, defines device functions only: no kernel to look for)

# a `__global__` definition with whatever stands between the keyword and `void` on its line (__launch_bounds__ with an expression,
# __attribute__((amdgpu_waves_per_eu(..)))); group 1: the template head in front of it, if any.  It stands on the headers' style:
# `__global__` and `void` on ONE line (a kernel with a line break between them is not matched; the host-header check below counts
# the keyword for that reason), and a template head counts only with nothing but whitespace and `inline` between it and
# `__global__` (a comment line in between makes a template count as non-template, which fails on the safe side).
_KERNEL = re.compile(r"(template\s*<[^;{}]*>\s*)?(?:inline\s+)?__global__\b[^\n;{]*?\bvoid\s+(\w+)\s*\(")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def header_kernels(header, templates=True):
    """Names of the `__global__` functions a header defines (templates=False: of those that are not templates)."""
    txt = _text(header)
    names = re.findall(r"__global__\s+(?:__launch_bounds__\(\w+\)\s+)?void\s+(\w+)\s*\(", txt)
    for head, name in _KERNEL.findall(txt):
        if name not in names:
            names.append(name)
    if not templates:
        names = [n for n in names if any(not head for head, name in _KERNEL.findall(txt) if name == n)]
    return names


def direct_includes(name):
    """The csrc headers a file includes by name."""
    return [h for h in re.findall(r'^#include "(\w+\.h)"', _text(name), re.M) if os.path.exists(os.path.join(CSRC, h))]


def cvd_kernel(mangled):
    """Plain name of a kernel in namespace cvd from its mangled name, None for any other."""
    m = re.match(r"_ZN3cvd(\d+)", mangled)
    return mangled[m.end():m.end() + int(m.group(1))] if m else None


def unit_asm(unit, tmp_path_factory):
    return device_asm(f'#include "{CSRC}/{unit}.hip"\n', tmp_path_factory.mktemp("codegen_" + unit), extra_flags=build.FLAGS)


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


def test_exchange_layer_emits_its_own_kernel_only(asm):
    names = kernel_names(asm)
    assert names
    assert [cvd_kernel(n) for n in names] == ["k_local_sum"] * len(names), names


def test_the_pattern_finds_attributed_and_template_kernels():
    """(what the checks below stand on: kernels behind an expression in __launch_bounds__ or an __attribute__, template or not)"""
    assert {"k_matvec_pairs_fast", "k_matvec_pairs"} <= set(header_kernels("cvd_kernels.h"))
    assert {"k_pcg_tail", "k_cg_update", "k_tl_rows_init"} <= set(header_kernels("cvd_pcg.h"))
    assert {"k_block_inverse_sweep", "k_block_inverse_mfma", "k_block_inverse"} <= set(header_kernels("cvd_block_inverse.h"))
    assert "k_cg_update" in header_kernels("cvd_pcg.h", templates=False)
    assert "k_pcg_tail" not in header_kernels("cvd_pcg.h", templates=False)


@pytest.mark.parametrize("unit", ["cvd_solve", "cvd_api", "cvd_temporal"])
def test_unit_emits_and_names_the_kernels_of_the_headers_it_includes(unit, tmp_path_factory):
    headers = [h for h in direct_includes(unit + ".hip") if header_kernels(h)]
    assert headers, unit
    defined = {k: h for h in headers for k in header_kernels(h)}
    emitted = [k for k in map(cvd_kernel, kernel_names(unit_asm(unit, tmp_path_factory))) if k is not None]
    assert emitted, unit
    for k in emitted:
        assert k in defined, (unit, k, "emitted, but no kernel header the unit includes by name defines it")
    text = re.sub(r"//[^\n]*", "", _text(unit + ".hip"))
    for h in headers:
        assert [k for k in header_kernels(h) if re.search(rf"\b{k}\b", text)], (unit, h, "included, but the unit names no kernel of it")


def test_host_header_brings_no_non_template_kernel():
    todo, seen = ["cvd_host.h"], []
    while todo:
        h = todo.pop()
        if h not in seen:
            seen.append(h)
            todo += direct_includes(h)
    assert "cvd_kernels.h" in seen and "cvd_device.h" in seen, seen
    for h in seen:
        assert header_kernels(h, templates=False) == [], h
        code = re.sub(r"//[^\n]*", "", _text(h))
        assert len(re.findall(r"\b__global__\b", code)) == len(_KERNEL.findall(code)), (h, "a __global__ the pattern does not match")
