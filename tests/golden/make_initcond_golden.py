"""Regenerates tests/golden/ic_r4.npz and ic_r8.npz: init_cond and the grid_initial_<nnn> files the reference's own
initial_cond_calc and initial_cond_output produce for the cases of flexpart_amd.synthetic.initcond_case().

The reference sources (par_mod, com_mod, point_mod, outg_mod, unc_mod, initial_cond_calc, initial_cond_output) are compiled
where they lie with flang (-cpp -O2 -mcmodel=medium; the r8 kind with -fdefault-real-8) together with our driver
tests/golden/ref_ic_driver.f90 into a build directory outside git (a temporary one unless --build-dir is given); nothing
of the reference is copied or written anywhere.  The fixtures hold init_cond after all calls (as the reference's real
kind) and the bytes of the files; the inputs are regenerated bit for bit by the tests.

    python tests/golden/make_initcond_golden.py
"""
import argparse
import glob
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
SOURCES = ("par_mod", "com_mod", "point_mod", "outg_mod", "unc_mod", "initial_cond_calc", "initial_cond_output")


def available():
    return os.path.isdir(REF) and os.access(FC, os.X_OK)


def build(kind, build_dir):
    """icref_<kind> in build_dir (built once: an existing binary newer than the driver is kept)."""
    d = os.path.join(build_dir, kind)
    exe = os.path.join(d, f"icref_{kind}")
    drv = os.path.join(HERE, "ref_ic_driver.f90")
    if os.path.exists(exe) and os.path.getmtime(exe) > os.path.getmtime(drv):
        return exe
    os.makedirs(d, exist_ok=True)
    flags = ["-cpp", "-O2", "-mcmodel=medium"] + (["-fdefault-real-8"] if kind == "r8" else [])
    objs = []
    for s in SOURCES:
        subprocess.check_call([FC, "-c"] + flags + [os.path.join(REF, s + ".f90"), "-o", s + ".o"], cwd=d)
        objs.append(s + ".o")
    subprocess.check_call([FC, "-c"] + flags + [drv, "-o", "ref_ic_driver.o"], cwd=d)
    subprocess.check_call([FC] + flags + ["ref_ic_driver.o"] + objs[::-1] + ["-o", exe], cwd=d)
    return exe


def write_input(c, fin):
    """The driver's input file for a synthetic.initcond_case()-shaped dict (the layout: ref_ic_driver.f90)."""
    nx, ny, nz = (int(v) for v in c["grid"])
    nxg, nyg, nzg = (int(v) for v in c["outgrid"])
    ns, mps, n = int(c["nspec"]), int(c["maxpointspec_act"]), int(c["npart"])
    with open(fin, "wb") as f:
        np.array([nx, ny, nz, n, nxg, nyg, nzg, ns, mps, int(c["ioutputforeachrelease"]), int(c["mdomainfill"]), int(c["linit_cond"]),
                  int(c["ind_rel"]), int(c["itime"]), int(c["memind"][0]), int(c["memind"][1])], np.int32).tofile(f)
        np.array(list(c["geom"]) + list(c["outgeom"]), np.float64).tofile(f)
        np.asarray(c["height"], np.float64).tofile(f)
        np.asarray(c["outheight"], np.float64).tofile(f)
        for m in range(2):
            np.ascontiguousarray(c["rho"][m], np.float64).tofile(f)        # [kz][jy][ix] = Fortran (ix,jy,kz)
        np.ascontiguousarray(np.asarray(c["xmass"], np.float64)[:, :mps]).tofile(f)      # [nspec][kp] = Fortran (kp,nspec)
        np.asarray(c["rho_rel"], np.float64).tofile(f)
        for k in ("xtra1", "ytra1", "ztra1"):
            np.asarray(c[k], np.float64).tofile(f)
        np.ascontiguousarray(c["xmass1"], np.float64).tofile(f)            # [nspec][n] = Fortran (n,nspec)
        np.asarray(c["npoint"], np.int32).tofile(f)
        np.asarray(c["itra1"], np.int32).tofile(f)


def run(exe, c, workdir):
    """One pass of the driver over a synthetic.initcond_case()-shaped dict: (init_cond as float64 shaped
    (kp, nspec, nz, ny, nx), the bytes of the grid_initial files by species)."""
    nxg, nyg, nzg = (int(v) for v in c["outgrid"])
    ns, mps = int(c["nspec"]), int(c["maxpointspec_act"])
    out = os.path.join(workdir, "out")
    os.makedirs(out, exist_ok=True)
    for f in glob.glob(os.path.join(out, "grid_initial_*")):
        os.remove(f)
    fin, fout = os.path.join(workdir, "ic_in.bin"), os.path.join(workdir, "ic_out.bin")
    write_input(c, fin)
    subprocess.check_call([exe, fin, fout, out + os.sep])
    grid = np.fromfile(fout, np.float64).reshape(mps, ns, nzg, nyg, nxg)
    files = []
    for ks in range(ns):
        with open(os.path.join(out, "grid_initial_%03d" % (ks + 1)), "rb") as f:
            files.append(f.read())
    assert len(glob.glob(os.path.join(out, "grid_initial_*"))) == ns
    return grid, files


def main():
    from flexpart_amd import synthetic as syn
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-dir", default=None)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference tree and flang are needed")
    bd = a.build_dir or tempfile.mkdtemp(prefix="icref_")
    for kind in ("r4", "r8"):
        exe = build(kind, bd)
        rec = {}
        for v in syn.IC_VARIANTS:
            grid, files = run(exe, syn.initcond_case(v), os.path.join(bd, kind))
            rec[f"init_cond_{v}"] = grid.astype(np.float32 if kind == "r4" else np.float64)
            for ks, data in enumerate(files):
                rec[f"file_{v}_{ks + 1}"] = np.frombuffer(data, np.uint8)
        np.savez_compressed(os.path.join(HERE, f"ic_{kind}.npz"), **rec)
        print("wrote", f"ic_{kind}.npz", os.path.getsize(os.path.join(HERE, f"ic_{kind}.npz")), "bytes")


if __name__ == "__main__":
    main()
