"""Regenerates tests/golden/cf_r4.npz and cf_r8.npz: the flux array and the grid_flux_* file the reference's own
calcfluxes and fluxoutput produce for the two cases of flexpart_amd.synthetic.calcfluxes_case().

The reference sources (par_mod, com_mod, outg_mod, flux_mod, caldate, calcfluxes, fluxoutput) are compiled where they lie
with flang (-cpp -O2 -mcmodel=medium; the r8 kind with -fdefault-real-8) together with our driver
tests/golden/ref_cf_driver.f90 into a build directory outside git (a temporary one unless --build-dir is given).  One
compile-time size differs from the shipped par_mod: maxageclass is 1 there ("maximum number of age classes used for
output", par_mod.f90:187-188 -- a user who wants age classes edits that line), and both lage(maxageclass) and the cell
counters of fluxoutput are sized with it, so the case's two age classes need it raised.  As oracle/build_ref.sh does for
its class variants, par_mod is piped through that one-line edit into the compiler; nothing of the reference is copied or
written anywhere.  The fixtures hold the flux array after all calls (as the reference's real kind) and the bytes of the
file; the inputs are regenerated bit for bit by the tests.

    python tests/golden/make_calcfluxes_golden.py
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
SOURCES = ("par_mod", "com_mod", "outg_mod", "flux_mod", "caldate", "calcfluxes", "fluxoutput")
SIZES = ("maxageclass=1,nclassunc=1\n", "maxageclass=4,nclassunc=1\n")


def available():
    return os.path.isdir(REF) and os.access(FC, os.X_OK)


def build(kind, build_dir):
    """cfref_<kind> in build_dir (built once: an existing binary newer than the driver is kept)."""
    d = os.path.join(build_dir, kind)
    exe = os.path.join(d, f"cfref_{kind}")
    drv = os.path.join(HERE, "ref_cf_driver.f90")
    if os.path.exists(exe) and os.path.getmtime(exe) > os.path.getmtime(drv):
        return exe
    os.makedirs(d, exist_ok=True)
    flags = ["-cpp", "-O2", "-mcmodel=medium"] + (["-fdefault-real-8"] if kind == "r8" else [])
    objs = []
    for s in SOURCES:
        src = os.path.join(REF, s + ".f90")
        if s == "par_mod":
            text = open(src).read()
            if text.count(SIZES[0]) != 1:
                sys.exit("par_mod has no 'maxageclass=1,nclassunc=1' line")
            subprocess.run([FC, "-c"] + flags + ["-x", "f95-cpp-input", "-", "-o", s + ".o"], cwd=d, check=True,
                           input=text.replace(SIZES[0], SIZES[1]).encode())
        else:
            subprocess.check_call([FC, "-c"] + flags + [src, "-o", s + ".o"], cwd=d)
        objs.append(s + ".o")
    subprocess.check_call([FC, "-c"] + flags + [drv, "-o", "ref_cf_driver.o"], cwd=d)
    subprocess.check_call([FC] + flags + ["ref_cf_driver.o"] + objs[::-1] + ["-o", exe], cwd=d)
    return exe


def run(exe, c, workdir):
    """One pass of the driver over a synthetic.calcfluxes_case()-shaped dict: (flux as float64 in the reference's element
    order reshaped to (nage, kp, nspec, nz, ny, nx, 6), the bytes of the grid_flux file, its name)."""
    nxg, nyg, nzg = (int(v) for v in c["outgrid"])
    ns, mps, lage, n = int(c["nspec"]), int(c["maxpointspec_act"]), np.asarray(c["lage"], np.int32), int(c["npart"])
    out = os.path.join(workdir, "out")
    os.makedirs(out, exist_ok=True)
    for f in glob.glob(os.path.join(out, "grid_flux_*")):
        os.remove(f)
    fin, fout = os.path.join(workdir, "cf_in.bin"), os.path.join(workdir, "cf_out.bin")
    with open(fin, "wb") as f:
        np.array([int(c["grid"][0]), nxg, nyg, nzg, ns, mps, int(c["ioutputforeachrelease"]), int(c["mdomainfill"]), lage.size], np.int32).tofile(f)
        lage.tofile(f)
        np.array([int(c["itime"]), int(c["ncalls"]), n], np.int32).tofile(f)
        np.array(list(c["geom"]) + list(c["outgeom"]) + [c["bdate"], c["outstep"]], np.float64).tofile(f)
        np.asarray(c["outheight"], np.float64).tofile(f)
        for k in ("area", "areaeast", "areanorth"):
            np.ascontiguousarray(c[k], np.float64).tofile(f)              # [kz][jy][ix] = Fortran (ix,jy,kz)
        for b in range(int(c["ncalls"])):
            np.stack([np.asarray(c[f"{k}{b}"], np.float64) for k in ("xold", "yold", "zold", "xnew", "ynew", "znew")]).tofile(f)
            np.ascontiguousarray(c[f"xmass1_{b}"], np.float64).tofile(f)  # [nspec][n] = Fortran (n,nspec)
            np.asarray(c[f"npoint{b}"], np.int32).tofile(f)
            np.asarray(c[f"itramem{b}"], np.int32).tofile(f)
    subprocess.check_call([exe, fin, fout, out + os.sep])
    flux = np.fromfile(fout, np.float64).reshape(lage.size, mps, ns, nzg, nyg, nxg, 6)
    files = glob.glob(os.path.join(out, "grid_flux_*"))
    assert len(files) == 1, files
    return flux, open(files[0], "rb").read(), os.path.basename(files[0])


def main():
    from flexpart_amd import synthetic as syn
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-dir", default=None)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference tree and flang are needed")
    bd = a.build_dir or tempfile.mkdtemp(prefix="cfref_")
    for kind in ("r4", "r8"):
        exe = build(kind, bd)
        rec = {}
        for v in syn.CF_VARIANTS:
            flux, data, name = run(exe, syn.calcfluxes_case(v), os.path.join(bd, kind))
            rec[f"flux_{v}"] = flux.astype(np.float32 if kind == "r4" else np.float64)
            rec[f"file_{v}"] = np.frombuffer(data, np.uint8)
            rec[f"name_{v}"] = np.array(name)
        np.savez_compressed(os.path.join(HERE, f"cf_{kind}.npz"), **rec)
        print("wrote", f"cf_{kind}.npz", os.path.getsize(os.path.join(HERE, f"cf_{kind}.npz")), "bytes")


if __name__ == "__main__":
    main()
