"""Regenerates tests/golden/gv_r4.npz and gv_r8.npz: the deposition velocities the reference's own getvdep returns for
the synthetic case of tests/getvdep_ref.py.

The unmodified reference sources (par_mod, com_mod, getvdep, getrb, getrc, raerod, psih, partdep, caldate, ew) are compiled
where they lie with flang (-O2 -mcmodel=medium; the r8 kind with -fdefault-real-8) together with our driver
tests/golden/ref_gv_driver.f90 into a build directory outside git (a temporary one unless --build-dir is given).  Nothing
of the reference is copied; the fixtures hold the inputs (synthetic, regenerated bit for bit by the tests) and the outputs.

    python tests/golden/make_getvdep_golden.py            # writes the two fixtures
    python tests/golden/make_getvdep_golden.py --time     # the reference's time per 361 x 181 wind field, 5 species, one core
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
REF = os.path.join(os.environ.get("FLEXPART_REFERENCE", "/root/reference"), "src")
FC = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
SOURCES = ("par_mod", "com_mod", "getvdep", "getrb", "getrc", "raerod", "psih", "partdep", "caldate", "ew")


def available():
    return os.path.isdir(REF) and os.access(FC, os.X_OK)


def build(kind, build_dir, modules_from=None):
    """gvref_<kind> in build_dir (built once: an existing binary newer than the driver is kept).  modules_from: a directory
    that already holds par_mod and com_mod compiled with the same flags (oracle/_ref/obj_<kind>): they are used, not rebuilt."""
    d = os.path.join(build_dir, kind)
    exe = os.path.join(d, f"gvref_{kind}")
    drv = os.path.join(HERE, "ref_gv_driver.f90")
    if os.path.exists(exe) and os.path.getmtime(exe) > os.path.getmtime(drv):
        return exe
    os.makedirs(d, exist_ok=True)
    flags = ["-cpp", "-O2", "-mcmodel=medium"] + (["-fdefault-real-8"] if kind == "r8" else [])
    have = modules_from is not None and all(os.path.exists(os.path.join(modules_from, m + e)) for m in SOURCES[:2] for e in (".o", ".mod"))
    inc = ["-I", modules_from] if have else []
    objs = []
    for s in SOURCES:
        if have and s in SOURCES[:2]:
            objs.append(os.path.join(modules_from, s + ".o"))
            continue
        subprocess.check_call([FC, "-c"] + flags + inc + [os.path.join(REF, s + ".f90"), "-o", s + ".o"], cwd=d)
        objs.append(s + ".o")
    subprocess.check_call([FC, "-c"] + flags + inc + [drv, "-o", "ref_gv_driver.o"], cwd=d)
    subprocess.check_call([FC] + flags + ["ref_gv_driver.o"] + objs + ["-o", exe], cwd=d)
    return exe


def run(exe, tables, gin, dy, ylat0, workdir, reps=0):
    """One pass of the driver: returns vdep [nspec][ny][nx] (and, with reps, the seconds per field it printed)."""
    import getvdep_ref as gr
    ny, nx = np.asarray(gin["ustar"]).shape
    nspec = int(tables["nspec"])
    fin, fout = os.path.join(workdir, "gv_in.bin"), os.path.join(workdir, "gv_out.bin")
    with open(fin, "wb") as f:
        np.array([nx, ny, nspec, int(gin["wftime"])], np.int32).tofile(f)
        np.array([tables["bdate"], dy, ylat0], np.float64).tofile(f)
        for k in gr.TABLES:
            np.ascontiguousarray(tables[k], np.float64).tofile(f)
        for k in gr.FIELDS:
            np.ascontiguousarray(gin[k], np.float64).tofile(f)
    out = subprocess.check_output([exe, fin, fout] + ([str(reps)] if reps else []), text=True)
    vdep = np.fromfile(fout, np.float64).reshape(nspec, ny, nx)
    if reps:
        return vdep, float(out.split()[-1])
    return vdep


def main():
    import getvdep_ref as gr
    from flexpart_amd import synthetic as syn
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference tree and flang are needed")
    bd = a.build_dir or tempfile.mkdtemp(prefix="gvref_")
    if a.time:
        nx, ny = 361, 181
        tables = syn.getvdep_tables(nx, ny, 5)
        gin = syn.getvdep_inputs((ny, nx))
        for kind in ("r4", "r8"):
            exe = build(kind, bd)
            secs = [run(exe, tables, gin, 1.0, -90.0, bd, reps=a.reps)[1] for _ in range(3)]
            print(f"{kind}: getvdep over {nx} x {ny} columns, 5 species, one core: {min(secs):.4f} s per wind field (three runs of {a.reps} passes: "
                  + ", ".join(f"{s:.4f}" for s in secs) + ")")
        return
    for kind in ("r4", "r8"):
        exe = build(kind, bd)
        rec = {}
        for t in range(len(syn.GV_WFTIMES)):
            tables, gin = gr.fixture_case(t)
            rec[f"vdep{t}"] = run(exe, tables, gin, gr.DY, gr.YLAT0, bd)
            rec[f"wftime{t}"] = np.int32(gin["wftime"])
            for k in gr.FIELDS:
                rec[f"{k}{t}"] = np.asarray(gin[k])
        for k in gr.TABLES:
            rec[k] = np.asarray(tables[k])
        rec["bdate"] = np.float64(tables["bdate"])
        np.savez_compressed(os.path.join(HERE, f"gv_{kind}.npz"), **rec)
        print("wrote", f"gv_{kind}.npz")


if __name__ == "__main__":
    main()
