#!/usr/bin/env python3
"""Is the device code of two source trees the same, function by function?

    tools/device_code_diff.py <parent-tree> <new-tree> [--scratch DIR] [--jobs N]

Each tree's six translation units (fpx_tu.hpp: r8p0 .. r4p2) are compiled to device assembly with the product flags
(HIPFLAGS of __graft_entry__, plus --cuda-device-only -S), the assembly is cut up by function symbol -- kernels and
out-of-line device functions -- and per symbol three texts are compared: the instructions, the .amdhsa_kernel descriptor
and the symbol's entry in .amdgpu_metadata.  Two things are normalised first, because they depend on what else the unit
holds and not on the function: the __hip_cuid_<hash> symbol, and the function's index inside compiler-local labels
(.LBB<i>_<n>, .Lfunc_end<i>, .LJTI<i>_<n>, .LCPI<i>_<n>, the unit-wide counter of .Lpost_getpc<i>; BB<i>_<n> where a
comment names a block, and the column at which such a comment starts).

Prints per unit the symbols only in the parent, only in the new tree, and the ones that differ; exit status 1 if any
symbol is new or differs (symbols that only the parent has are for the reader to judge), 2 if a compile failed.
A tree from before the split compiles fpx_engine.hip with -DFPX_TU_PART; one after it compiles the three sources.
CPU only: nothing is run on a GPU.  With --scratch the assembly is kept there, else it goes to a temporary directory.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIPCC, HIPFLAGS  # noqa: E402

SOURCES = {0: "fpx_engine.hip", 1: "fpx_step_prep.hip", 2: "fpx_step_loop.hip"}


def units(tree):
    """(name, compile command without the output) of the six units of a tree"""
    csrc = os.path.join(tree, "flexpart_amd", "csrc")
    split = os.path.exists(os.path.join(csrc, SOURCES[1]))
    for rb in (8, 4):
        for part in (0, 1, 2):
            if split:
                args = [f"-DFPX_TU_REAL={rb}", os.path.join(csrc, SOURCES[part])]
            else:
                args = [f"-DFPX_TU_REAL={rb}", f"-DFPX_TU_PART={part}", os.path.join(csrc, "fpx_engine.hip")]
            yield f"r{rb}p{part}", [HIPCC] + HIPFLAGS + ["--cuda-device-only", "-S"] + args


LOCAL = re.compile(r"(\.L[A-Za-z_]+?|\bBB)(\d+)(_\d+)?\b")   # .LBB12_3, .Lfunc_end12, .Lpost_getpc40; BB12_3 as the comments name a block


def normalise(line):
    line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", line)
    line = LOCAL.sub(lambda m: m.group(1) + "#" + (m.group(3) or ""), line)
    return re.sub(r"\s+;", " ;", line)     # the column of a comment moves with the length of the label in front of it


def split_assembly(path):
    """{symbol: {"code": [...], "descriptor": [...], "metadata": [...]}} of one assembly file"""
    lines = [normalise(l.rstrip()) for l in open(path)]
    n = len(lines)
    syms = {}
    functions = {m.group(1) for l in lines for m in [re.match(r"\s*\.type\s+([^,\s]+),@function", l)] if m}
    i = 0
    while i < n:
        m = re.match(r"(\S+):", lines[i])
        if m and m.group(1) in functions:
            # instructions: from the label to .Lfunc_end, and the resource figures (.set <symbol>.num_vgpr ...) behind it, up to
            # the next section; the descriptor, which sits in between in a section of its own, is taken out
            j = i
            while j < n and not lines[j].startswith(".Lfunc_end"):
                j += 1
            while j < n and not lines[j].lstrip().startswith(".section"):
                j += 1
            code, inside = [], False
            for l in lines[i:j]:
                inside = inside or l.strip().startswith(".amdhsa_kernel ")
                if not inside:
                    code.append(l)
                inside = inside and l.strip() != ".end_amdhsa_kernel"
            syms.setdefault(m.group(1), {})["code"] = code
            i = j
        else:
            i += 1
    i = 0
    while i < n:
        if lines[i].strip().startswith(".amdhsa_kernel "):                # kernel descriptor
            j = i
            while lines[j].strip() != ".end_amdhsa_kernel":
                j += 1
            syms.setdefault(lines[i].split()[1], {})["descriptor"] = lines[i:j + 1]
            i = j
        i += 1
    if "\t.amdgpu_metadata" in lines:                                     # one list entry per kernel under amdhsa.kernels:
        i = lines.index("\t.amdgpu_metadata")
        entry = []
        for l in lines[i:lines.index("\t.end_amdgpu_metadata")] + ["end"]:
            if l.startswith("    ") and entry:
                entry.append(l)
                continue
            for e in entry:
                k = re.match(r"(?:    |  - )\.name:\s+(\S+)$", e)
                if k:
                    syms.setdefault(k.group(1), {})["metadata"] = entry
            entry = [l] if l.startswith("  - ") else []
    return syms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--scratch", help="directory for the assembly (kept); default: a temporary one")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1), help="compiles at a time (at most 16)")
    a = ap.parse_args()
    scratch = a.scratch or tempfile.mkdtemp(prefix="device_code_diff_")
    os.makedirs(scratch, exist_ok=True)

    jobs = []
    for side, tree in (("parent", a.parent), ("new", a.new)):
        for name, cmd in units(os.path.abspath(tree)):
            jobs.append((side, name, cmd + ["-o", os.path.join(scratch, f"{side}_{name}.s")]))

    def run(job):
        print("[compile]", job[0], job[1], flush=True)
        return subprocess.call(job[2])

    with ThreadPoolExecutor(max(1, min(16, a.jobs))) as pool:
        failed = [j[:2] for j, rc in zip(jobs, pool.map(run, jobs)) if rc != 0]
    if failed:
        print("compile failed:", failed)
        return 2

    bad = report(scratch, [j[1] for j in jobs if j[0] == "parent"])
    if not a.scratch:
        shutil.rmtree(scratch)
    return 1 if bad else 0


def report(scratch, names):
    bad = False
    for name in names:
        old = split_assembly(os.path.join(scratch, f"parent_{name}.s"))
        new = split_assembly(os.path.join(scratch, f"new_{name}.s"))
        only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
        differ = sorted(s for s in set(old) & set(new) if old[s] != new[s])
        print(f"== {name}: {len(old)} symbols in the parent, {len(new)} in the new tree, {len(set(old) & set(new)) - len(differ)} identical")
        for title, names in (("only in the parent", only_old), ("only in the new tree", only_new), ("differ", differ)):
            print(f"   {title}: {len(names)}")
            for s in names:
                what = "" if title != "differ" else "  [" + ", ".join(k for k in ("code", "descriptor", "metadata") if old[s].get(k) != new[s].get(k)) + "]"
                print(f"      {s}{what}")
        bad = bad or bool(only_new or differ)
    return bad


if __name__ == "__main__":
    sys.exit(main())
