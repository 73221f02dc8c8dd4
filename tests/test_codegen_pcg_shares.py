"""Code-generation guards of the pair product's shares mode (no GPU needed: hipcc cross-compiles gfx950).

k_matvec_pairs_fast<KD, NT, SPEC, false, true> sums the r^T z shares the fused PCG tail left behind in its prologue and closes the
previous iteration's scalars (cvd_kernels.h).  The product's constraint loop is f64-VALU-bound at 128 VGPRs and 31 SGPR spill slots:
the new prologue work must not tax it.  Every shares instantiation a launch can select is compiled beside its twin (SHARES = false)
in ONE unit -- instantiations of a template perturb each other's register allocation, so only twins of one unit compare -- and read
off the assembly:

  * the register budget: <= 128 VGPRs, no spilled vector register, no scratch;
  * the segment that holds the constraint loop -- what a wave can execute between the prologue's last barrier and the reduction's
    first -- has the twin's counts of f64 instructions and of LDS f64 atomics, and no more instructions or SGPR lane saves /
    restores (v_writelane / v_readlane) than the twin;
  * the default path through the prologue (CoarseView::Wb == nullptr: the fused coarse gather is jumped over) has no more full
    vector-memory waits than the twin's.

The segments are taken from the control-flow graph, not from the text between two `s_barrier` lines: the compiler lays cold blocks
(workgroup 0's bookkeeping stores, the fused coarse gather) out wherever it likes, also between the loop and the reduction.
One-wave workgroups (the deterministic build's <4, 64, 1>) compile without any barrier: only their budget is checked.

Figures of the tree as committed (twin / shares): <4,256,1> 1190 / 1169 instructions, 72 / 65 lane operations; <4,128,1> 1176 / 1166,
71 / 65; f64 and ds_add_f64 counts are equal; the default path has no full vector wait in front of the first barrier on either side.
The Global level's <1,256,1> is NOT among the instantiations a launch can select (launchMatvec builds the shares form for KD = 4
only; Global-level solves keep the closing tail): every form of it that was compiled -- some 700 variants of the prologue, DESIGN_LOG.md
-- had at least 3 instructions and 9 lane restores more than its twin's 1029 / 48 in the per-direction set-up of its loop segment, which
is the tax this file exists to keep out.  The Huber variant's forms (SPEC = 2) are not built either: <4,256,2> needs 128 VGPRs with one
spilled (8 B of scratch; twin 124, none) and <4,128,2> has 90 lane operations in its loop segment against its twin's 85; solves with
robust_loss = 1 keep the closing tail.
"""
import re

import pytest

from tests.codegen_util import CSRC, device_asm, kernel_info, kernel_names

SIG = ("(Layout, Table, Items, const double*, const FrameConst*, const double*, const double*, const double*, const double*, int, "
       "double*, CoarseView)")
# (KD, NT, SPEC) of the list-mode instantiations launchMatvec selects in shares mode: ALL of them (productSumsShares and the launch
# macro of cvd_matvec.hip admit KD = 4 and SPEC = 1 only; 64 threads is the deterministic build's workgroup)
INSTANCES = [(4, 256, 1), (4, 128, 1), (4, 64, 1)]
WITH_BARRIERS = [i for i in INSTANCES if i[1] > 64]

SOURCE = f'''
#include <hip/hip_runtime.h>
#include "{CSRC}/cvd_device.h"
#include "{CSRC}/cvd_kernels.h"
namespace cvd {{
''' + "".join(f"template __global__ void k_matvec_pairs_fast<{kd}, {nt}, {spec}, false, {sh}>{SIG};\n"
              for kd, nt, spec in INSTANCES for sh in ("false", "true")) + "}\n"

INSTR = re.compile(r"^\s+([a-z]\w*)")


class Cfg:
    """Basic blocks of a kernel body: lists of (mnemonic, line), successors by index."""

    def __init__(self, body):
        self.blocks, self.label_at, succ_label = [[]], {}, {}
        for line in body.split("\n"):
            lab = re.match(r"^(\.LBB\d+_\d+):", line)
            if lab:
                if self.blocks[-1]:
                    self.blocks.append([])
                self.label_at[lab.group(1)] = len(self.blocks) - 1
                if "Loop Header" in line:
                    self.blocks[-1].append(("loop_header", line))
                continue
            m = INSTR.match(line)
            if not m:
                continue
            self.blocks[-1].append((m.group(1), line))
            if m.group(1).startswith(("s_branch", "s_cbranch", "s_endpgm")):
                succ_label[len(self.blocks) - 1] = (m.group(1), line.split()[-1])
                self.blocks.append([])
        self.succ = []
        for i in range(len(self.blocks)):
            kind, target = succ_label.get(i, (None, None))
            nxt = [i + 1] if i + 1 < len(self.blocks) else []
            if kind is None:
                self.succ.append(nxt)
            elif kind == "s_endpgm":
                self.succ.append([])
            elif kind == "s_branch":
                self.succ.append([self.label_at[target]])
            else:
                self.succ.append([self.label_at[target]] + nxt)   # (taken, fall-through)

    def barrier_positions(self):
        return [(b, k) for b, blk in enumerate(self.blocks) for k, (mn, _) in enumerate(blk) if mn == "s_barrier"]

    def region(self, start, cut=None):
        """Instructions a wave can execute from position `start` = (block, index) before it meets an `s_barrier`.  cut: a
        (block, successor) edge that is not followed."""
        out, seen, todo = [], set(), [start]
        while todo:
            b, k = todo.pop()
            if (b, k) in seen:
                continue
            seen.add((b, k))
            stopped = False
            for mn, line in self.blocks[b][k:]:
                if mn == "s_barrier":
                    stopped = True
                    break
                out.append((mn, line))
            if not stopped:
                todo += [(s, 0) for s in self.succ[b] if (b, s) != cut]
        return out

    def reaches_loop(self, b):
        return any(mn == "loop_header" for mn, _ in self.region((b, 0)))


def figures(instrs):
    names = [mn for mn, _ in instrs if mn != "loop_header"]
    return {"instructions": len(names), "f64": sum(1 for n in names if re.match(r"v_\w+_f64", n)),
            "ds_add_f64": sum(1 for n in names if n.startswith("ds_add_f64")),
            "lane": sum(1 for n in names if n.startswith(("v_writelane", "v_readlane")))}


def loop_segment(body):
    """Between the prologue's last barrier (the third in the text: the one behind the shared-intrinsics fix-up is conditional) and
    whatever barrier comes next on any path."""
    cfg = Cfg(body)
    bars = cfg.barrier_positions()
    assert len(bars) >= 4
    b, k = bars[2]
    seg = cfg.region((b, k + 1))
    assert any(mn == "loop_header" for mn, _ in seg), "the constraint loop lies behind the prologue's last barrier"
    return figures(seg)


def default_prologue_full_waits(body):
    """Full vector waits on the default path from the kernel's entry to its first barrier: at the one uniform branch of which exactly
    one side runs into a loop in front of the barrier (the fused coarse gather's), only the other side is followed."""
    cfg = Cfg(body)
    cut = []
    for b in range(len(cfg.blocks)):
        if len(cfg.succ[b]) == 2 and cfg.blocks[b][-1][0] in ("s_cbranch_vccnz", "s_cbranch_vccz", "s_cbranch_scc0", "s_cbranch_scc1"):
            loops = [cfg.reaches_loop(s) for s in cfg.succ[b]]
            if loops[0] != loops[1]:
                cut.append((b, cfg.succ[b][loops.index(True)]))
                break   # (the first one from the top: the gather's own branches lie behind it)
    assert cut, "no uniform branch around the fused coarse gather found"
    path = cfg.region((0, 0), cut=cut[0])
    assert not any(mn == "loop_header" for mn, _ in path)
    return sum(1 for mn, line in path if mn == "s_waitcnt" and "vmcnt(0)" in line)


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    return device_asm(SOURCE, tmp_path_factory.mktemp("codegen_pcg_shares"), extra_flags=("-munsafe-fp-atomics",))


def _name(inst, shares):
    kd, nt, spec = inst
    return f"19k_matvec_pairs_fastILi{kd}ELi{nt}ELi{spec}ELb0ELb{int(shares)}E"


def _kernel(asm, inst, shares):
    """(descriptor fields, metadata entry) of the instantiation; the entry is cut out here: kernel_info's spans every kernel of the
    unit in front of the one asked for."""
    fields, _body, _meta = kernel_info(asm, _name(inst, shares))
    mangled, = [n for n in kernel_names(asm) if _name(inst, shares) in n]
    entry, = [e for e in asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count:") if re.search(r"\.name:\s+" + re.escape(mangled) + r"\n", e)]
    return fields, entry


def _whole_body(asm, inst, shares):
    """The kernel's text to the end of the function (kernel_info stops at the first s_endpgm: early exits and cold blocks lie behind)."""
    mangled, = [n for n in kernel_names(asm) if _name(inst, shares) in n]
    body = asm[asm.index(f"\n{mangled}:"):]
    return body[:body.index(".Lfunc_end")]


ids = lambda i: "kd%d-nt%d-spec%d" % i   # noqa: E731


@pytest.mark.parametrize("inst", INSTANCES, ids=ids)
def test_shares_register_budget(asm, inst):
    fields, meta = _kernel(asm, inst, True)
    spilled = re.search(r"\.vgpr_spill_count:\s*(\d+)", meta)
    sgpr = re.search(r"\.sgpr_spill_count:\s*(\d+)", meta)
    print(f"{inst}: next_free_vgpr {fields['next_free_vgpr']}, scratch {fields['private_segment_fixed_size']} B, "
          f"{sgpr.group(1) if sgpr else '?'} SGPR spill slots (lane writes, not memory)")
    assert fields["next_free_vgpr"] <= 128, fields
    assert spilled is not None and int(spilled.group(1)) == 0, meta
    assert fields["private_segment_fixed_size"] == 0, fields


@pytest.mark.parametrize("inst", WITH_BARRIERS, ids=ids)
def test_shares_do_not_tax_the_constraint_loop(asm, inst):
    twin, mine = (loop_segment(_whole_body(asm, inst, sh)) for sh in (False, True))
    print(f"{inst}: twin {twin}, shares {mine}")
    assert mine["f64"] == twin["f64"] and mine["ds_add_f64"] == twin["ds_add_f64"], (twin, mine)
    assert mine["instructions"] <= twin["instructions"], (twin, mine)
    assert mine["lane"] <= twin["lane"], (twin, mine)


@pytest.mark.parametrize("inst", WITH_BARRIERS, ids=ids)
def test_shares_default_prologue_has_no_more_full_waits(asm, inst):
    twin, mine = (default_prologue_full_waits(_whole_body(asm, inst, sh)) for sh in (False, True))
    print(f"{inst}: full vector waits on the default path in front of the first barrier: twin {twin}, shares {mine}")
    assert mine <= twin
