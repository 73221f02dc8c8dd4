#!/usr/bin/env python3
"""CPU only: is a source change a change of machine code?  Device assembly of the solver's translation units, compared kernel by kernel
between two trees (a refactor of device code should leave every kernel `identical`).
  isa_compare.py dump OUTDIR [--root TREE]     compile every unit of TREE (default: this tree) with build.FLAGS -S --cuda-device-only,
                                               once plain and once with -DCVD_DETERMINISTIC=1, into OUTDIR/<build>/<unit>.s
  isa_compare.py compare PARENT_DIR CHANGE_DIR one line per kernel symbol per build: `identical`, or the code-object figures of both
                                               sides (VGPR / AGPR / SGPR, spills, scratch and LDS bytes, instructions of the body)
The comparison is a plain text diff after dropping comments and the .file / .ident lines."""
import argparse
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robust_cvd_amd import build as b  # noqa: E402

UNITS = ["cvd_eval", "cvd_matvec", "cvd_precond", "cvd_solve", "cvd_temporal", "cvd_setup", "cvd_api"]
BUILDS = {"plain": [], "det": ["-DCVD_DETERMINISTIC=1"]}
FIGURES = [("vgpr", "vgpr_count"), ("agpr", "agpr_count"), ("sgpr", "sgpr_count"), ("vgpr_spill", "vgpr_spill_count"),
           ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size")]


def dump(outdir, root, units=UNITS):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    jobs = []
    for name, defs in BUILDS.items():
        os.makedirs(os.path.join(outdir, name), exist_ok=True)
        for u in units:
            jobs.append([hipcc] + b.FLAGS + defs + ["-S", "--cuda-device-only", os.path.join(root, "robust_cvd_amd", "csrc", u + ".hip"),
                                                    "-o", os.path.join(outdir, name, u + ".s")])
    with ThreadPoolExecutor(max_workers=min(len(jobs), 16, os.cpu_count() or 1)) as pool:
        list(pool.map(subprocess.check_call, jobs))


def clean(lines):
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if ln and not ln.lstrip().startswith((".file", ".ident")):
            out.append(ln)
    return out


def kernels(path):
    """{symbol: (cleaned body + kernel descriptor, figures)} of one assembly file."""
    with open(path) as f:
        txt = f.read()
    lines = txt.split("\n")
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target)", txt, re.S):
        blk = m.group(0)
        sym = re.search(r"\.symbol:\s+(\S+)\.kd", blk).group(1)
        if not sym.startswith("_ZN3cvd"):  # (library instantiations the units pull in: not this project's kernels)
            continue
        meta[sym] = {k: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1)) for k, key in FIGURES}
    out = {}
    for sym in meta:
        i0 = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
        i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))  # (the kernel descriptor lies in between)
        body = clean(lines[i0:i1])
        fig = dict(meta[sym])
        fig["instructions"] = sum(1 for ln in body if ln.startswith("\t") and not ln.lstrip().startswith("."))
        out[sym] = (body, fig)
    return out


def compare(pa, ch):
    differ = 0
    for name in BUILDS:
        for u in UNITS:
            ka, kb = kernels(os.path.join(pa, name, u + ".s")), kernels(os.path.join(ch, name, u + ".s"))
            for sym in sorted(set(ka) | set(kb)):
                if sym not in ka or sym not in kb:
                    verdict = "only in " + ("parent" if sym in ka else "change")
                elif ka[sym][0] == kb[sym][0]:
                    verdict = "identical"
                else:
                    verdict = "DIFFERS parent " + " ".join(f"{k}={v}" for k, v in ka[sym][1].items()) + \
                              " | change " + " ".join(f"{k}={v}" for k, v in kb[sym][1].items())
                differ += verdict != "identical"
                print(name, u, sym, verdict)
    print(f"# {differ} kernel(s) not identical")
    return differ


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("outdir")
    d.add_argument("--root", default=ROOT)
    c = sub.add_parser("compare")
    c.add_argument("parent")
    c.add_argument("change")
    a = ap.parse_args()
    if a.cmd == "dump":
        dump(a.outdir, a.root)
    else:
        sys.exit(1 if compare(a.parent, a.change) else 0)
