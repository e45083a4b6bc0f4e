"""Regenerates tests/golden/gvn_r4.npz and gvn_r8.npz: the deposition velocities the reference's own getvdep_nests
returns for the synthetic nest case of tests/nestpar_ref.py.

The unmodified reference sources (par_mod_meteoswiss -- the reference's own variant with maxnests = 1 --, com_mod,
getvdep_nests, getrb, getrc, raerod, psih, partdep, caldate, ew) are compiled where they lie with flang (-O2
-mcmodel=medium; the r8 kind with -fdefault-real-8) together with our driver tests/golden/ref_gvn_driver.f90 into a build
directory outside git (a temporary one unless --build-dir is given).  Nothing of the reference is copied; the fixtures hold
the inputs (synthetic, regenerated bit for bit by the tests) and the outputs.

    python tests/golden/make_getvdep_nests_golden.py            # writes the two fixtures
    python tests/golden/make_getvdep_nests_golden.py --time     # the reference's time per 571 x 301 nest field, 5 species, one core
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
MODULES = (("par_mod", "par_mod_meteoswiss"), ("com_mod", "com_mod"))
SOURCES = ("getvdep_nests", "getrb", "getrc", "raerod", "psih", "partdep", "caldate", "ew")


def available():
    return os.path.isdir(REF) and os.access(FC, os.X_OK)


def build(kind, build_dir, modules_from=None):
    """gvnref_<kind> in build_dir (built once: an existing binary newer than the driver is kept).  modules_from: a directory
    that already holds par_mod (the maxnests = 1 variant) and com_mod compiled with the same flags (oracle/_ref/obj_<kind>n)."""
    d = os.path.join(build_dir, kind + "n")
    exe = os.path.join(d, f"gvnref_{kind}")
    drv = os.path.join(HERE, "ref_gvn_driver.f90")
    if os.path.exists(exe) and os.path.getmtime(exe) > os.path.getmtime(drv):
        return exe
    os.makedirs(d, exist_ok=True)
    flags = ["-cpp", "-O2", "-mcmodel=medium"] + (["-fdefault-real-8"] if kind == "r8" else []) + ["-DFLEXREF_NESTS"]
    have = modules_from is not None and all(os.path.exists(os.path.join(modules_from, m + e)) for m, _ in MODULES for e in (".o", ".mod"))
    inc = ["-I", modules_from] if have else []
    objs = []
    for mod, src in MODULES:
        if have:
            objs.append(os.path.join(modules_from, mod + ".o"))
            continue
        subprocess.check_call([FC, "-c"] + flags + [os.path.join(REF, src + ".f90"), "-o", mod + ".o"], cwd=d)
        objs.append(mod + ".o")
    for s in SOURCES:
        subprocess.check_call([FC, "-c"] + flags + inc + [os.path.join(REF, s + ".f90"), "-o", s + ".o"], cwd=d)
        objs.append(s + ".o")
    subprocess.check_call([FC, "-c"] + flags + inc + [drv, "-o", "ref_gvn_driver.o"], cwd=d)
    subprocess.check_call([FC] + flags + ["ref_gvn_driver.o"] + objs + ["-o", exe], cwd=d)
    return exe


def run(exe, tables, gin, dy, ylat0, dyn, ylat0n, workdir, reps=0):
    """One pass of the driver: returns vdepn [nspec][nyn][nxn] (and, with reps, the seconds per field it printed).
    dy, ylat0: the mother grid's; dyn, ylat0n: the nest's own (set in com_mod, not read by getvdep_nests)."""
    import getvdep_ref as gr
    ny, nx = np.asarray(gin["ustar"]).shape
    nspec = int(tables["nspec"])
    fin, fout = os.path.join(workdir, "gvn_in.bin"), os.path.join(workdir, "gvn_out.bin")
    with open(fin, "wb") as f:
        np.array([nx, ny, nspec, int(gin["wftime"])], np.int32).tofile(f)
        np.array([tables["bdate"], dy, ylat0, dyn, ylat0n], np.float64).tofile(f)
        for k in gr.TABLES:
            np.ascontiguousarray(tables[k], np.float64).tofile(f)
        for k in gr.FIELDS:
            np.ascontiguousarray(gin[k], np.float64).tofile(f)
    out = subprocess.check_output([exe, fin, fout] + ([str(reps)] if reps else []), text=True)
    vdep = np.fromfile(fout, np.float64).reshape(nspec, ny, nx)
    if reps:
        return vdep, float(out.split()[-1])
    return vdep


def time_reference(build_dir, reps=5, nx=571, ny=301, nspec=5):
    """{kind: seconds per nest wind field} of the reference's getvdep_nests on one core at the reference's own nest size
    (par_mod_meteoswiss.f90:154), the best of three runs of `reps` passes."""
    from flexpart_amd import synthetic as syn
    tables = syn.getvdep_tables(nx, ny, nspec, seed=4150)
    gin = syn.nest_getvdep_inputs((ny, nx))
    res = {}
    for kind in ("r4", "r8"):
        exe = build(kind, build_dir)
        res[kind] = [run(exe, tables, gin, 1.0, -90.0, 0.02, 40.0, build_dir, reps=reps)[1] for _ in range(3)]
    return res


def main():
    import nestpar_ref as nr
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference tree and flang are needed")
    bd = a.build_dir or tempfile.mkdtemp(prefix="gvnref_")
    if a.time:
        for kind, secs in time_reference(bd, a.reps).items():
            print(f"{kind}: getvdep_nests over 571 x 301 columns, 5 species, one core: {min(secs):.4f} s per wind field (three runs of {a.reps} passes: "
                  + ", ".join(f"{s:.4f}" for s in secs) + ")")
        return
    from flexpart_amd import synthetic as syn
    for kind in ("r4", "r8"):
        exe = build(kind, bd)
        rec = {}
        for t in range(len(syn.GV_WFTIMES)):
            tables, gin = nr.fixture_case(t)
            rec[f"vdep{t}"] = run(exe, tables, gin, nr.GEOM[1], nr.GEOM[3], nr.NESTGEOM[1], nr.NESTGEOM[3], bd)
            rec[f"wftime{t}"] = np.int32(gin["wftime"])
            for k in nr.FIELDS:
                rec[f"{k}{t}"] = np.asarray(gin[k])
        for k in nr.TABLES:
            rec[k] = np.asarray(tables[k])
        rec["bdate"] = np.float64(tables["bdate"])
        np.savez_compressed(os.path.join(HERE, f"gvn_{kind}.npz"), **rec)
        print("wrote", f"gvn_{kind}.npz")


if __name__ == "__main__":
    main()
