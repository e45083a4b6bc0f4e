"""Regenerates tests/golden/pv_r4.npz and pv_r8.npz: the potential vorticity the reference's own calcpv and calcpv_nests
return for the three cases of flexpart_amd.synthetic.calcpv_case().

The unmodified reference sources (par_mod, com_mod, calcpv; for the nest case par_mod_meteoswiss -- the reference's own
maxnests = 1 sizes -- com_mod, calcpv_nests) are compiled where they lie with flang (-cpp -O2 -mcmodel=medium; the r8 kind
with -fdefault-real-8) together with our driver tests/golden/ref_pv_driver.f90 into a build directory outside git (a
temporary one unless --build-dir is given).  Both routines keep two automatic arrays of the full par_mod size (36 MB each
in r4, 72 MB in r8) on the stack, so the binary runs with the stack limit raised.  Nothing of the reference is copied;
the fixtures hold the inputs (synthetic, regenerated bit for bit by the tests), pvh per case and the record of decisions
of the restatement tests/calcpv_ref.py (which bracket every search ended in), from which the tests count branch coverage.

    python tests/golden/make_calcpv_golden.py            # writes the two fixtures
    python tests/golden/make_calcpv_golden.py --time     # the reference's seconds per 361 x 181 x 138 field, one core
"""
import argparse
import os
import resource
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
REF = os.path.join(os.environ.get("FLEXPART_REFERENCE", "/root/reference"), "src")
FC = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
INPUTS = ("akz", "bkz", "ps", "tth", "uuh", "vvh")


def available():
    return os.path.isdir(REF) and os.access(FC, os.X_OK)


def build(kind, build_dir, nest=False, modules_from=None):
    """pvref_<kind>[n] in build_dir (built once: an existing binary newer than the driver is kept).  modules_from: a
    directory that already holds par_mod and com_mod compiled with the same flags (oracle/_ref/obj_<kind>[n])."""
    tag = kind + ("n" if nest else "")
    d = os.path.join(build_dir, tag)
    exe = os.path.join(d, f"pvref_{tag}")
    drv = os.path.join(HERE, "ref_pv_driver.f90")
    if os.path.exists(exe) and os.path.getmtime(exe) > os.path.getmtime(drv):
        return exe
    os.makedirs(d, exist_ok=True)
    flags = ["-cpp", "-O2", "-mcmodel=medium"] + (["-fdefault-real-8"] if kind == "r8" else []) + (["-DFLEXREF_NESTS"] if nest else [])
    have = modules_from is not None and all(os.path.exists(os.path.join(modules_from, m + e)) for m in ("par_mod", "com_mod") for e in (".o", ".mod"))
    inc = ["-I", modules_from] if have else []
    objs = []
    for mod, src in (("par_mod", "par_mod_meteoswiss" if nest else "par_mod"), ("com_mod", "com_mod")):
        if have:
            objs.append(os.path.join(modules_from, mod + ".o"))
            continue
        subprocess.check_call([FC, "-c"] + flags + [os.path.join(REF, src + ".f90"), "-o", mod + ".o"], cwd=d)
        objs.append(mod + ".o")
    sub = "calcpv_nests" if nest else "calcpv"
    subprocess.check_call([FC, "-c"] + flags + inc + [os.path.join(REF, sub + ".f90"), "-o", sub + ".o"], cwd=d)
    subprocess.check_call([FC, "-c"] + flags + inc + [drv, "-o", "ref_pv_driver.o"], cwd=d)
    subprocess.check_call([FC] + flags + ["ref_pv_driver.o", sub + ".o"] + objs + ["-o", exe], cwd=d)
    return exe


def _raise_stack():
    hard = resource.getrlimit(resource.RLIMIT_STACK)[1]
    resource.setrlimit(resource.RLIMIT_STACK, (hard, hard))


def run(exe, c, workdir, reps=0):
    """One pass of the driver over a synthetic.calcpv_case()-shaped dict: returns pvh [nz][ny][nx] (and, with reps, the
    seconds per call it printed)."""
    nx, ny, nz = (int(v) for v in c["grid"])
    fin, fout = os.path.join(workdir, "pv_in.bin"), os.path.join(workdir, "pv_out.bin")
    with open(fin, "wb") as f:
        np.array([nx, ny, nz] + [int(v) for v in c["globalflags"]], np.int32).tofile(f)
        np.array([c["geom"][0], c["geom"][1], c["geom"][3]], np.float64).tofile(f)
        for k in INPUTS:
            np.ascontiguousarray(c[k], np.float64).tofile(f)
    out = subprocess.check_output([exe, fin, fout] + ([str(reps)] if reps else []), text=True, preexec_fn=_raise_stack)
    pvh = np.fromfile(fout, np.float64).reshape(nz, ny, nx)
    if reps:
        return pvh, float(out.split()[-1])
    return pvh


def main():
    import calcpv_ref as pr
    from flexpart_amd import synthetic as syn
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference tree and flang are needed")
    bd = a.build_dir or tempfile.mkdtemp(prefix="pvref_")
    if a.time:
        m = syn.model_levels(361, 181, 138, global_grid=True, polar=True)
        for kind in ("r4", "r8"):
            exe = build(kind, bd)
            secs = [run(exe, m, bd, reps=a.reps)[1] for _ in range(3)]
            print(f"{kind}: calcpv over 361 x 181 x 138, one core: {min(secs):.4f} s per wind field (three runs of {a.reps} calls: "
                  + ", ".join(f"{s:.4f}" for s in secs) + ")")
        return
    for kind in ("r4", "r8"):
        store = np.float32 if kind == "r4" else np.float64          # r4 values are exact in float32: half the file
        rec = {}
        for name in syn.PV_CASES:
            c = syn.calcpv_case(name)
            exe = build(kind, bd, nest=(name == "nest"))
            rec[f"pvh_{name}"] = run(exe, c, bd).astype(store)
            rec[f"code_{name}"] = pr.calcpv_ref(c, kind)["code"]
            if name == "limited":                                    # 'nest' runs on the same arrays, 'global' on them with
                for k in INPUTS:                                     # column nx-1 overwritten by column 0
                    rec[k] = np.asarray(c[k])
            rec[f"geom_{name}"] = np.asarray(c["geom"])
        np.savez_compressed(os.path.join(HERE, f"pv_{kind}.npz"), **rec)
        print("wrote", f"pv_{kind}.npz", os.path.getsize(os.path.join(HERE, f"pv_{kind}.npz")), "bytes")


if __name__ == "__main__":
    main()
