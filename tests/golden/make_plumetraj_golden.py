"""Regenerates tests/golden/pt_r4.npz and pt_r8.npz: the records the reference's own plumetraj (with clustering,
centerofmass, distance, distance2 and mean_mod) appends to trajectories.txt for the cases of
flexpart_amd.synthetic.plumetraj_case().

The reference sources are compiled where they lie with flang (-cpp -O2 -mcmodel=medium; the r8 kind with
-fdefault-real-8) together with our driver tests/golden/ref_pt_driver.f90 into a build directory outside git (a temporary
one unless --build-dir is given); nothing of the reference is copied or written anywhere.  plumetraj keeps three
automatic arrays of maxpart reals on the stack (and clustering one of integers): the driver runs with the stack limit
raised to the hard limit.  The fixtures hold the bytes of the records; the inputs are regenerated bit for bit by the tests.

    python tests/golden/make_plumetraj_golden.py
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
SOURCES = ("par_mod", "com_mod", "point_mod", "mean_mod", "plumetraj", "clustering", "centerofmass", "distance", "distance2")


def available():
    return os.path.isdir(REF) and os.access(FC, os.X_OK)


def build(kind, build_dir):
    """ptref_<kind> in build_dir (built once: an existing binary newer than the driver is kept)."""
    d = os.path.join(build_dir, kind)
    exe = os.path.join(d, f"ptref_{kind}")
    drv = os.path.join(HERE, "ref_pt_driver.f90")
    if os.path.exists(exe) and os.path.getmtime(exe) > os.path.getmtime(drv):
        return exe
    os.makedirs(d, exist_ok=True)
    flags = ["-cpp", "-O2", "-mcmodel=medium"] + (["-fdefault-real-8"] if kind == "r8" else [])
    objs = []
    for s in SOURCES:
        subprocess.check_call([FC, "-c"] + flags + [os.path.join(REF, s + ".f90"), "-o", s + ".o"], cwd=d)
        objs.append(s + ".o")
    subprocess.check_call([FC, "-c"] + flags + [drv, "-o", "ref_pt_driver.o"], cwd=d)
    subprocess.check_call([FC] + flags + ["ref_pt_driver.o"] + objs[::-1] + ["-o", exe], cwd=d)
    return exe


def write_input(c, itime, fin):
    """The driver's input file for a synthetic.plumetraj_case()-shaped dict (the layout: ref_pt_driver.f90)."""
    nx, ny, nz = (int(v) for v in c["grid"])
    n = int(np.asarray(c["xtra1"]).size)
    with open(fin, "wb") as f:
        np.array([nx, ny, nz, n, int(np.asarray(c["ireleasestart"]).size), int(itime), int(c["memind"][0]), int(c["memind"][1]),
                  int(c["memtime"][0]), int(c["memtime"][1]), int(np.asarray(c["lage"]).ravel()[-1])], np.int32).tofile(f)
        np.asarray(c["geom"], np.float64).tofile(f)
        np.asarray(c["height"], np.float64).tofile(f)
        np.ascontiguousarray(c["oro"], np.float64).tofile(f)               # [jy][ix] = Fortran (ix,jy)
        for m in range(2):
            np.ascontiguousarray(c["pv"][m], np.float64).tofile(f)         # [kz][jy][ix] = Fortran (ix,jy,kz)
            np.ascontiguousarray(c["hmix"][m], np.float64).tofile(f)
            np.ascontiguousarray(c["tropopause"][m], np.float64).tofile(f)
        for k in ("xtra1", "ytra1", "ztra1"):
            np.asarray(c[k], np.float64).tofile(f)
        for k in ("npoint", "itra1", "ireleasestart", "ireleaseend"):
            np.asarray(c[k], np.int32).tofile(f)


def _raise_stack():
    soft, hard = resource.getrlimit(resource.RLIMIT_STACK)
    resource.setrlimit(resource.RLIMIT_STACK, (hard, hard))


def run(exe, c, itime, workdir):
    """One call of plumetraj for a synthetic.plumetraj_case()-shaped dict: the bytes of the records."""
    fin, fout = os.path.join(workdir, "pt_in.bin"), os.path.join(workdir, "trajectories.txt")
    write_input(c, itime, fin)
    subprocess.check_call([exe, fin, fout], preexec_fn=_raise_stack)
    with open(fout, "rb") as f:
        return f.read()


def main():
    from flexpart_amd import synthetic as syn
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-dir", default=None)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference tree and flang are needed")
    bd = a.build_dir or tempfile.mkdtemp(prefix="ptref_")
    for kind in ("r4", "r8"):
        exe = build(kind, bd)
        rec = {}
        for v in syn.PT_VARIANTS:
            c = syn.plumetraj_case(v)
            rec[f"records_{v}"] = np.frombuffer(run(exe, c, int(c["itime"]), os.path.join(bd, kind)), np.uint8)
        np.savez_compressed(os.path.join(HERE, f"pt_{kind}.npz"), **rec)
        print("wrote", f"pt_{kind}.npz", os.path.getsize(os.path.join(HERE, f"pt_{kind}.npz")), "bytes")


if __name__ == "__main__":
    main()
